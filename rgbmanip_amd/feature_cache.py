"""The estimator's two PSPNet feature caches: `SlotFeatureCache` keeps one record per entry of a frame pool the
caller names (`estimate_device_indexed(..., fresh=...)`), `ContentFeatureCache` keys records by the prepared crop's content
(`estimate` / `estimate_device`, feature_keys.py).  Both answer with `CachedViews`: what `AdaPoseNet.forward_cached` reads."""
from __future__ import annotations

from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .adapose import prepare_inputs
from .feature_keys import FeatureKeyTable


class CachedViews(NamedTuple):
    pool: torch.Tensor                    # [records, feature_bytes]
    slot1: torch.Tensor                   # [n] int32: the record of pose i's view 1
    slot2: torch.Tensor
    ok: Optional[torch.Tensor]            # [n] bool: both records hold the pose's frames; None: all of them do


class SlotFeatureCache:
    """One record per frame-pool entry; nothing is allocated before the first `update`."""

    def __init__(self, net, normalize=True):
        self.net = net
        self.normalize = bool(normalize)  # the estimator's image transform: records must hold the maps of the crops its network is fed
        self.pool = None                  # [M + 1, feature_bytes]: one record per frame-pool entry; record M = the all-zero crop's map
        self.valid = None                 # [M + 1] bool on the device: record holds the map of the entry's current frame (M: always)
        self._fresh_dev = {}              # fresh tuple -> (entries, identity intrinsics) on the device
        self.views_computed = 0

    def invalidate(self):
        if self.valid is not None:
            self.valid[:-1] = False

    def update(self, rgb_pool, mask_pool, S, fresh, map1, map2, prepare_seed) -> CachedViews:
        """Compute the records of the `fresh` pool entries; the records the poses of map1 / map2 read and whether both are valid."""
        net, dev = self.net, self.net.device
        M = int(rgb_pool.shape[0])
        if self.pool is None or self.pool.shape != (M + 1, net.feature_bytes):
            self.pool = self.valid = None
            self.pool = net.feature_pool(M + 1)
            self.valid = torch.zeros(M + 1, dtype=torch.bool, device=dev)
            # record M: the map of an all-zero crop, read in place of a missing view (map entry < 0) or of an entry without a valid record
            net.features(torch.zeros(1, 3, S, S, dtype=torch.float32, device=dev), torch.full((1,), M, dtype=torch.int32, device=dev), self.pool)
            self.valid[M] = True
        fresh = [int(e) for e in fresh]
        if fresh:
            if min(fresh) < 0 or max(fresh) >= M:
                raise ValueError(f"estimate_device_indexed: fresh entries must lie in [0, {M}), got {min(fresh)} .. {max(fresh)}")
            key = tuple(fresh)
            fd = self._fresh_dev.get(key)
            if fd is None:
                if len(self._fresh_dev) >= 64:
                    self._fresh_dev.clear()
                # the crop windows' intrinsics are not needed for the image: any K serves this preparation
                fd = self._fresh_dev[key] = (torch.as_tensor(np.asarray(fresh, dtype=np.int32)).to(dev),
                                             torch.eye(3, dtype=torch.float64, device=dev).expand(len(fresh), 3, 3).contiguous())
            img = prepare_inputs(rgb_pool, mask_pool, fd[1], S, 1024, prepare_seed, frame_map=fd[0], normalize=self.normalize)["img"]
            net.features(img, fd[0], self.pool)
            self.valid[fd[0].long()] = True
            self.views_computed += len(fresh)
        slots = []
        for m in (map1, map2):
            m = torch.as_tensor(m).to(device=dev, dtype=torch.int64)
            slots.append(torch.where((m < 0) | (m > M), torch.full_like(m, M), m))
        ok = self.valid[slots[0]] & self.valid[slots[1]]
        s1, s2 = (torch.where(self.valid[m], m, torch.full_like(m, M)).to(torch.int32) for m in slots)
        return CachedViews(self.pool, s1, s2, ok)


# what `ContentFeatureCache.keys` enqueued: the two prepared views, their crops, the keys on the device and in pinned host memory
# (complete once `ev` has), and the stream all of it was enqueued on
PendingKeys = namedtuple("PendingKeys", "a b img keys_dev keys ev stream")


class ContentFeatureCache:
    """Records keyed by crop content; pool and table are built by the first `reserve`."""

    def __init__(self, net, records_cfg):
        self.net = net
        self.records_cfg = int(records_cfg)       # 0: twice the poses of the largest call so far
        self.pool = None                          # [records, feature_bytes]
        self.table = None                         # FeatureKeyTable(records), built with the pool
        self._tie = None                          # (feature_bytes, options) the records were written under
        self._poses = 0                           # poses of the largest call so far
        self.views_computed = 0
        self.bypassed = 0                         # calls / chunks with more distinct crops than the pool has records (run on the plain path)

    def invalidate(self):
        if self.table is not None:
            self.table.clear()

    def reserve(self, n):
        """The pool and the table for calls of up to n poses; both start empty when the pool is (re)allocated: a larger call than any
        before (hip_feature_cache_records: 0), or a net whose record size or options changed (records are not interchangeable)."""
        net = self.net
        self._poses = max(self._poses, int(n))
        records = self.records_cfg or 2 * self._poses
        tie = (net.feature_bytes, tuple(sorted(net.options.items())))
        if self.pool is None or self.pool.shape[0] != records or self._tie != tie:
            self.pool = None
            self.pool = net.feature_pool(records)
            self.table = FeatureKeyTable(records)
            self._tie = tie

    def keys(self, a, b) -> PendingKeys:
        """Enqueue on the current stream: fingerprint of cat(img1, img2) and the copy of the [2n,2] keys to pinned host memory."""
        img = torch.cat((a["img"], b["img"]))
        V = int(img.shape[0])
        keys = torch.empty(V, 2, dtype=torch.int64, device=img.device)
        _lib.check(_lib.load().rgbm_crop_fingerprint(_lib.ptr(img), V, int(img[0].numel()), _lib.ptr(keys), _lib.stream_ptr()),
                   "rgbm_crop_fingerprint")
        host = torch.empty(V, 2, dtype=torch.int64, pin_memory=True)
        host.copy_(keys, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return PendingKeys(a, b, img, keys, host, ev, torch.cuda.current_stream(img.device))

    def finish(self, pend: PendingKeys) -> Optional[CachedViews]:
        """Wait for the keys of `keys` (the host waits for that stream's work up to the key copy, nothing else), assign record slots and
        run the PSPNet on the crops not met before, on the current stream.  None: more distinct crops than records (counted in
        `bypassed`), the caller runs the plain path."""
        img = pend.img
        dev = img.device
        cur = torch.cuda.current_stream(dev)
        pend.ev.synchronize()
        if cur != pend.stream:
            cur.wait_event(pend.ev)
            for t in [img, pend.keys_dev] + [v for d in (pend.a, pend.b) for v in d.values() if isinstance(v, torch.Tensor)]:
                t.record_stream(cur)                      # allocated on the other stream: not to be handed out again while this one reads
        n = int(img.shape[0]) // 2
        got = self.table.assign(pend.keys.numpy().view(np.uint64))
        if got is None:
            self.bypassed += 1
            return None
        slots, compute = got
        # slot tables and miss lists go up in one copy from pinned memory (a pageable copy would block the host until the stream has drained)
        m = len(compute)
        tab = torch.empty(2 * n + 2 * m, dtype=torch.int32, pin_memory=True)
        tab_np = tab.numpy()
        tab_np[: 2 * n] = slots
        if m:
            tab_np[2 * n:] = np.asarray(compute, dtype=np.int32).T.reshape(-1)
        tab_d = tab.to(dev, non_blocking=True)
        if m:
            whole = m == 2 * n and [v for v, _ in compute] == list(range(2 * n))
            miss = img if whole else img.index_select(0, tab_d[2 * n: 2 * n + m])
            self.net.features(miss, tab_d[2 * n + m:], self.pool)
            self.views_computed += m
        return CachedViews(self.pool, tab_d[:n], tab_d[n: 2 * n], None)

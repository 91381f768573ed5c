"""Content keys of prepared crops and the host table that turns them into feature-record slots ("content keys").

`estimate()` gets its frames as fresh arrays on every call (rl_pose.py:189-223 copies them out of the queue), so a frame has no
identity but its content.  The PSPNet's feature map depends on the prepared crop img[v] ([3,S,S] fp32) and nothing else: the device
hashes that crop (`rgbm_crop_fingerprint`, include/rgbm.h) into two 64-bit words, the host keeps key -> record slot here.

`crop_keys` is the numpy restatement of the kernel's definition, word for word; `FeatureKeyTable` is pure Python and needs no GPU."""
from __future__ import annotations

import numpy as np

SEEDS = (0x9E3779B97F4A7C15, 0xD1B54A32D192ED03)
_M1, _M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def crop_keys(words) -> np.ndarray:
    """[V, 2] uint64 keys of V rows of 32-bit words (any 4-byte dtype, [V, ...]; one row if 1-D): for k in {0, 1}

        x = (uint64(bits(w_i)) | uint64(i) << 32) ^ SEEDS[k]
        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
        key[v][k] = sum_i x  mod 2^64

    The bit pattern is hashed, not the value (+0.0 and -0.0 differ); integer arithmetic only, so any summation order gives these bits."""
    w = np.ascontiguousarray(words)
    if w.dtype.itemsize != 4:
        raise TypeError(f"crop_keys: rows of 32-bit words, got {w.dtype}")
    w = w.view(np.uint32).reshape((w.shape[0], -1) if w.ndim > 1 else (1, -1))
    if w.shape[1] < 1:
        raise ValueError("crop_keys: at least one word per row")
    base = w.astype(np.uint64) | (np.arange(w.shape[1], dtype=np.uint64) << np.uint64(32))[None]
    keys = np.empty((w.shape[0], 2), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k, seed in enumerate(SEEDS):
            x = base ^ np.uint64(seed)
            x ^= x >> np.uint64(30); x *= np.uint64(_M1)
            x ^= x >> np.uint64(27); x *= np.uint64(_M2)
            x ^= x >> np.uint64(31)
            keys[:, k] = x.sum(axis=1, dtype=np.uint64)
    return keys


class FeatureKeyTable:
    """key -> slot of a pool of `records` feature records, least recently used out first.

    `assign(keys)` takes the [V, 2] uint64 keys of one call (or one chunk of it) and returns `(slots, compute)`: slots [V] int32, the
    record of every view, and compute, the (view, slot) pairs whose records are not in the pool yet and must be written before the
    slots are read.  A key already in the table is a hit; equal keys inside one call share one slot and appear in compute once (the
    first view that carries them); new keys take free slots first (lowest first), then the slots whose last use lies furthest back
    (calls are the clock; equal age: lowest slot) — never a slot this call refers to.  A call with more distinct keys than the table
    has records cannot be served: `assign` returns None and changes nothing (the caller runs it on the plain path).  The table only
    names slots; it trusts the caller to write every record in compute before the next `assign`."""

    def __init__(self, records: int):
        self.records = int(records)
        if self.records < 1:
            raise ValueError(f"FeatureKeyTable: at least one record, got {records}")
        self.clear()

    def clear(self):
        """Forget every key: all slots are free again."""
        self._slot_of = {}                               # (key0, key1) -> slot
        self._key_of = [None] * self.records             # slot -> key, None = free
        self._used = [0] * self.records                  # slot -> clock of the last call that referred to it
        self._clock = 0

    def __len__(self):
        return len(self._slot_of)

    def __contains__(self, key):
        return (int(key[0]), int(key[1])) in self._slot_of

    def assign(self, keys):
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 2)
        ks = [(int(a), int(b)) for a, b in keys.tolist()]
        first = {}                                       # distinct key -> first view that carries it, in order of appearance
        for v, k in enumerate(ks):
            first.setdefault(k, v)
        if len(first) > self.records:
            return None
        self._clock += 1
        held = {self._slot_of[k] for k in first if k in self._slot_of}
        new = [k for k in first if k not in self._slot_of]
        compute = []
        if new:
            free = [s for s in range(self.records) if self._key_of[s] is None]
            if len(free) < len(new):
                old = sorted((s for s in range(self.records) if self._key_of[s] is not None and s not in held),
                             key=lambda s: (self._used[s], s))
                free += old[: len(new) - len(free)]
            for k, s in zip(new, free):
                if self._key_of[s] is not None:
                    del self._slot_of[self._key_of[s]]
                self._key_of[s] = k
                self._slot_of[k] = s
                compute.append((first[k], s))
        slots = np.fromiter((self._slot_of[k] for k in ks), dtype=np.int32, count=len(ks))
        for s in set(slots.tolist()):
            self._used[s] = self._clock
        return slots, compute

"""Host frames and masks -> HBM: the conversion on the way into pinned staging (`stage_rows`), the double-buffered staging ring, the
whole-array uploads (`frames_to_device` / `masks_to_device`), the crop-window upload of cfg hip_upload: "windows" (`mask_windows`,
`pack_windows`, `WindowRing`) and the chunk pipeline of `estimate()` (`ChunkPipeline`)."""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

_HOST_THREADS = max(1, min(32, (os.cpu_count() or 1)))
_POOL = None


def _host_pool():
    """Thread pool of the host-side frame conversion (created on first use)."""
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=_HOST_THREADS, thread_name_prefix="rgbm-upload")
    return _POOL


def _cast_into(dst, src):
    """dst[...] = src cast to dst's dtype (float64 / float16 frames -> float32 staging; same dtype: a plain copy).  numpy releases the GIL."""
    np.copyto(dst, src, casting="same_kind")


def _nonzero_into(dst_u8, src):
    np.not_equal(src, 0, out=dst_u8.view(np.bool_))


def _split(n, parts):
    """[lo, hi) ranges cutting n rows into at most `parts` nearly equal pieces"""
    parts = max(1, min(parts, n))
    return [(n * i // parts, n * (i + 1) // parts) for i in range(parts)]


def host_array(x):
    return x.numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(np.asarray(x))


def _frame_dtype(src):
    """What frames are staged as: uint8 crosses as bytes, float frames as float32."""
    if src.dtype == np.uint8:
        return torch.uint8
    if src.dtype.kind != "f":
        raise TypeError(f"estimate: rgb frames must be float images in [0, 1] or uint8, got {src.dtype}")
    return torch.float32


def stage_rows(dst_np, src, lo, hi, kind, pool, parts=None):
    """dst_np[: hi - lo] = rows [lo, hi) of src, converted on the way, split over `pool` in at most `parts` (default: every host
    thread) pieces; returns the pieces' futures.  kind "frame": a casting copy to dst's dtype — float frames are converted to float32
    WHILE they are copied into the pinned staging buffers (numpy's casting copy is as fast as its plain copy once a pool of threads
    runs it: both are bound by host memory, tools/host_convert_bw.py), so float64 frames cross PCIe at half their size; uint8 stays
    uint8.  kind "mask": non-zero = object, one 0 / 1 byte per pixel crosses PCIe (bool: the same bytes, copied)."""
    if kind == "frame":
        _frame_dtype(src)
        fn = _cast_into
    elif src.dtype == np.bool_:
        fn, src = np.copyto, src.view(np.uint8)
    else:
        fn = _nonzero_into
    return [pool.submit(fn, dst_np[p:q], src[lo + p:lo + q]) for p, q in _split(hi - lo, parts or _HOST_THREADS)]


class StagingRing:
    """Two slots of pinned host buffers (one per array of `shapes` / `dtypes`, `rows` rows each) with their device twins and the
    event of each slot's last host -> device copy.  `key` is what it was built for: the owner builds another when that changes."""

    def __init__(self, rows, shapes, dtypes, device):
        self.key = (rows, tuple(shapes), tuple(dtypes), device)
        self.rows, self.device = rows, device
        self.pin = [[torch.empty((rows,) + tuple(s), dtype=t, pin_memory=True) for s, t in zip(shapes, dtypes)] for _ in range(2)]
        self.host = [[t.numpy() for t in slot] for slot in self.pin]              # the pinned buffers as numpy arrays
        self.dev = [[torch.empty((rows,) + tuple(s), dtype=t, device=device) for s, t in zip(shapes, dtypes)] for _ in range(2)]
        self.h2d = [torch.cuda.Event(), torch.cuda.Event()]
        self.used = [False, False]

    @classmethod
    def matching(cls, ring, rows, shapes, dtypes, device):
        return ring if ring is not None and ring.key == (rows, tuple(shapes), tuple(dtypes), device) else cls(rows, shapes, dtypes, device)

    @property
    def pinned_bytes(self):
        return sum(t.numel() * t.element_size() for slot in self.pin for t in slot)

    def wait(self, slot):
        if self.used[slot]:
            self.h2d[slot].synchronize()                   # the copy that last read this slot's pinned buffers has finished

    def stage(self, slot, srcs, lo, hi, kinds, parts=None):
        """Host threads: rows [lo, hi) of every source into the slot's pinned buffers (after `wait`)."""
        pool = _host_pool()
        for f in [f for dst, src, kind in zip(self.host[slot], srcs, kinds) for f in stage_rows(dst, src, lo, hi, kind, pool, parts)]:
            f.result()

    def copy(self, slot, rows):
        """Start the slot's copy on the current stream and record its event; returns the device buffers' first `rows` rows."""
        for d, p in zip(self.dev[slot], self.pin[slot]):
            d[:rows].copy_(p[:rows], non_blocking=True)
        self.h2d[slot].record()
        self.used[slot] = True
        return [d[:rows] for d in self.dev[slot]]


def frames_to_device(frames, device, ring, chunk_bytes, keep_u8=False):
    """[N,H,W,3] host frames (float64 / float32 in [0,1], or uint8) -> CUDA float32 [N,H,W,3] in [0,1]; with `keep_u8`, uint8 frames
    (host or CUDA) stay uint8 on the device — `prepare_inputs` reads bytes as the same pixel values (rgbm_prepare_inputs_u8), so the
    float32 copy and its pass over the frames are not needed.  Frames that already are CUDA tensors pass through.  A pool of host
    threads copies each chunk into one of two pinned staging buffers while the previous chunk's copy is in flight; float frames are cast to float32 by that copy (3.8 GB of float64 frames arrive per call at N = 256 and
    cross PCIe as 1.9 GB), uint8 frames cross as bytes and are scaled on the device (or kept, `keep_u8`).  Returns (frames, the ring to hand in next time)."""
    if isinstance(frames, torch.Tensor) and frames.is_cuda:      # (device-side dtype conversion of an uploaded chunk)
        if keep_u8 and frames.dtype == torch.uint8:
            return frames, ring
        return (frames.to(torch.float32) if frames.dtype != torch.uint8 else (frames.to(torch.float64) / 255.0).to(torch.float32)), ring
    src = host_array(frames)
    tdt = _frame_dtype(src)                                # float frames: converted to float32 by the staging copy itself
    n = src.shape[0]
    per = max(1, int(np.prod(src.shape[1:]))) * (1 if src.dtype == np.uint8 else 4)
    rows = max(1, min(n, chunk_bytes // per))
    ring = StagingRing.matching(ring, rows, [src.shape[1:]], [tdt], device)
    as_bytes = keep_u8 and src.dtype == np.uint8
    out = torch.empty(tuple(src.shape), dtype=torch.uint8 if as_bytes else torch.float32, device=device)
    for i, a in enumerate(range(0, n, rows)):
        b, k = min(a + rows, n), i & 1
        ring.wait(k)
        ring.stage(k, [src], a, b, ["frame"])
        d, = ring.copy(k, b - a)
        # stream-ordered: this conversion runs before the copy that next overwrites the slot's device buffer (two chunks later)
        if src.dtype == np.uint8 and not as_bytes:
            # x / 255 through float64: torch's float32 division on ROCm is not correctly rounded (126 of the 256 byte values
            # differ from numpy's float32(x) / float32(255) by one ulp, tools/check_div.py); the float64 quotient rounded to
            # float32 equals the correctly rounded float32 quotient for every byte value
            out[a:b].copy_(d.to(torch.float64) / 255.0)
        else:
            out[a:b].copy_(d)
    return out, ring


def masks_to_device(masks, device):
    """[N,H,W] host masks (bool / uint8 / any number type, non-zero = object) -> CUDA uint8."""
    if isinstance(masks, torch.Tensor) and masks.is_cuda:
        return masks
    m = masks if isinstance(masks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(masks)))
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    elif m.dtype != torch.uint8:
        m = m.ne(0).view(torch.uint8)                              # multi-threaded on the host: 1 byte per pixel crosses PCIe
    return m.to(device, non_blocking=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# hip_upload: "windows" — only each frame's crop window crosses PCIe.  The crop kernel reads the square window get_bbox derives from the
# mask (40 .. 440 pixels on a side of a 480 x 640 frame); the host derives the same window, packs that part of the frame and of the mask
# back to back into pinned staging and `rgbm_prepare_inputs_windows` prepares the network inputs from the packed pixels, bit for bit
# what `rgbm_prepare_inputs_opt` writes from the whole frames.
WINDOW_MAX = 440                      # get_bbox's largest window side (lib/utils.py:10-38)
WINDOW_EMPTY = (0, 40, 0, 40)         # what mask_window_kernel uses for an empty mask


def _mask_extents(m):
    """Rows and columns of m [n,H,W] (uint8 / bool) that hold a non-zero pixel: ([n,H] bool, [n,W] bool).  OR-reductions: down the
    columns a SIMD loop over whole rows, along the rows over 8 pixels at a time where the rows are 8-byte words."""
    m = m.view(np.uint8) if m.dtype == np.bool_ else m
    cols = np.bitwise_or.reduce(m, axis=1) != 0
    wide = m.view(np.uint64) if m.flags.c_contiguous and m.shape[2] % 8 == 0 else m
    rows = np.bitwise_or.reduce(wide, axis=2) != 0
    return rows, cols


def mask_windows(mask_bytes):
    """mask_bytes [N,H,W] uint8 (or bool), non-zero = object -> (window [N,4] int32 = rmin, rmax, cmin, cmax; valid [N] int32).
    The window `mask_window_kernel` (csrc/prepare.hip) derives on the device: the mask's row / column extents, then the integer
    arithmetic of get_bbox (lib/utils.py:10-38) with H and W in place of 480 and 640 — a square of side (longer extent // 40 + 1) * 40,
    at most 440, centred on the extent and shifted back into the frame.  An empty mask: (0, 40, 0, 40) and valid 0."""
    m = np.asarray(mask_bytes)
    if m.ndim != 3 or m.dtype not in (np.uint8, np.bool_):
        raise TypeError(f"mask_windows: [N,H,W] uint8 or bool masks, got {m.dtype} {m.shape}")
    n, H, W = m.shape
    if H < WINDOW_MAX or W < WINDOW_MAX:
        raise ValueError(f"mask_windows: frames must be at least {WINDOW_MAX} x {WINDOW_MAX} (a smaller frame cannot hold the crop window), got {H} x {W}")
    rows, cols = _mask_extents(m)
    valid = rows.any(axis=1)
    y1, y2 = rows.argmax(axis=1).astype(np.int64), H - 1 - rows[:, ::-1].argmax(axis=1).astype(np.int64)
    x1, x2 = cols.argmax(axis=1).astype(np.int64), W - 1 - cols[:, ::-1].argmax(axis=1).astype(np.int64)
    win = np.minimum((np.maximum(y2 - y1, x2 - x1) // 40 + 1) * 40, WINDOW_MAX)
    cy, cx = (y1 + y2) // 2, (x1 + x2) // 2
    rmin, rmax, cmin, cmax = cy - win // 2, cy + win // 2, cx - win // 2, cx + win // 2
    rmax, rmin = np.where(rmin < 0, rmax - rmin, rmax), np.maximum(rmin, 0)
    cmax, cmin = np.where(cmin < 0, cmax - cmin, cmax), np.maximum(cmin, 0)
    rmin, rmax = np.where(rmax > H, rmin - (rmax - H), rmin), np.minimum(rmax, H)
    cmin, cmax = np.where(cmax > W, cmin - (cmax - W), cmin), np.minimum(cmax, W)
    window = np.stack([rmin, rmax, cmin, cmax], axis=1)
    window[~valid] = WINDOW_EMPTY
    return window.astype(np.int32), valid.astype(np.int32)


def mask_windows_pooled(mask_bytes, pool, parts=None):
    """`mask_windows` with the frames cut into pieces of at least 16 for the threads of `pool`: the reductions stream the masks once
    and release the GIL, a single thread is bound by its own memory bandwidth (5 GB/s: 30 ms per view at 256 poses); smaller pieces
    cost more in handing tasks over than they save (a 32-pose chunk: two pieces per view).  Returns the pieces' futures;
    `gather_windows` joins their results."""
    n = len(mask_bytes)
    return [pool.submit(mask_windows, mask_bytes[p:q]) for p, q in _split(n, min(parts or _HOST_THREADS, max(1, n // 16)))]


def gather_windows(futures):
    res = [f.result() for f in futures]
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def window_offsets(window):
    """Exclusive prefix sum of h * w over window [N,4] -> (offset [N] int64, total pixels)."""
    area = (window[:, 1] - window[:, 0]).astype(np.int64) * (window[:, 3] - window[:, 2]).astype(np.int64)
    offset = np.zeros(len(area), dtype=np.int64)
    np.cumsum(area[:-1], out=offset[1:])
    return offset, int(area.sum())


def _pack_one(pix, mpix, frame, mask, win, off):
    """One frame: its window of the frame (casting copy) and of the mask (non-zero -> 1) into the packed buffers at pixel offset `off`."""
    rmin, rmax, cmin, cmax = win
    h, w = rmax - rmin, cmax - cmin
    np.copyto(pix[3 * off: 3 * (off + h * w)].reshape(h, w, 3), frame[rmin:rmax, cmin:cmax], casting="same_kind")
    np.not_equal(mask[rmin:rmax, cmin:cmax], 0, out=mpix[off: off + h * w].reshape(h, w).view(np.bool_))


def _pack_range(pix, mpix, frames, masks, lo, window, offset, p, q):
    for f in range(p, q):
        _pack_one(pix, mpix, frames[lo + f], masks[lo + f], window[f], offset[f])


def pack_windows(pix, mpix, frames, masks, lo, hi, window, offset, pool=None, parts=None):
    """Frames [lo, hi) of `frames` [N,H,W,3] (float: cast to pix's float32; uint8: bytes kept) and of `masks` [N,H,W] (any number type
    or bool) -> the packed buffers `pix` (flat, 3 elements per pixel) and `mpix` (flat uint8): frame lo + f's window `window[f]` row-major
    at pixel offset `offset[f]`.  One casting copy per frame and array; with `pool` (the upload thread pool) the frames are cut into at
    most `parts` (default: every host thread) runs of at least 8, one task each — a task per frame spends more time handing tasks over than
    copying —
    and the tasks' futures are returned for the caller to wait on; without a pool the copies run here."""
    if masks.dtype == np.bool_:
        masks = masks.view(np.uint8)
    window, offset = [tuple(int(v) for v in w) for w in window[: hi - lo]], [int(o) for o in offset[: hi - lo]]
    if pool is None:
        _pack_range(pix, mpix, frames, masks, lo, window, offset, 0, hi - lo)
        return []
    parts = min(parts or _HOST_THREADS, max(1, (hi - lo) // 8))         # runs of at least 8 frames
    return [pool.submit(_pack_range, pix, mpix, frames, masks, lo, window, offset, p, q) for p, q in _split(hi - lo, parts)]


class PackedViews:
    """What `WindowRing.copy` hands on: per view v (0, 1) the packed device buffers and tables of `rows` poses, and the frames' size."""

    def __init__(self, pix, mask, offset, window, valid, H, W):
        self.pix, self.mask, self.offset, self.window, self.valid, self.H, self.W = pix, mask, offset, window, valid, H, W


class WindowRing:
    """`StagingRing` for packed crop windows: `slots` slots of pinned host buffers with their device twins — per view a pixel buffer of
    rows * 440 * 440 * 3 elements (float32, or uint8 for byte frames) and a mask buffer of rows * 440 * 440 bytes, i.e. a slot capacity of
    rows * 440^2 * (3 * px_bytes + 1) bytes per view — and one table (offsets int64, windows int32, valid int32 of both views).  `stage`
    derives the windows of poses [lo, hi) from the masks and packs them, `copy` moves the used prefix of every buffer and the table.
    Masks that are neither uint8 nor bool are first reduced to bytes (`stage_rows`, one read of the source as in the whole-frame path)
    in a host buffer that never leaves the host.  `payload_bytes` / `table_bytes` count what `copy` has handed to the copy engine."""

    def __init__(self, rows, frame_dtypes, device, slots=2):
        self.key = ("windows", rows, tuple(frame_dtypes), device, slots)
        self.rows, self.device = rows, device
        on_gpu = torch.device(device).type == "cuda"
        cap = rows * WINDOW_MAX * WINDOW_MAX
        tab_bytes = 2 * rows * (8 + 16 + 4)

        def buffers(**kw):
            return [[torch.empty(3 * cap, dtype=t, **kw) for t in frame_dtypes] + [torch.empty(cap, dtype=torch.uint8, **kw) for _ in range(2)] +
                    [torch.empty(tab_bytes, dtype=torch.uint8, **kw)] for _ in range(slots)]
        self.pin = buffers(pin_memory=on_gpu)
        self.host = [[t.numpy() for t in slot] for slot in self.pin]
        self.dev = buffers(device=device)
        self.h2d = [torch.cuda.Event() if on_gpu else None for _ in range(slots)]
        self.used = [False] * slots
        self.totals = [(0, 0)] * slots            # packed pixels of view 1 / view 2 in each slot
        self.shape = [None] * slots               # (H, W) of the frames packed into each slot
        self._mask_bytes = None                   # [2, rows, H, W] uint8: masks of another number type, reduced to bytes (host only)
        self.payload_bytes = self.table_bytes = 0

    @classmethod
    def matching(cls, ring, rows, srcs, device, slots=2, grow=False):
        """`ring` if it serves these host arrays (rgb1, rgb2, mask1, mask2) at `rows` poses per slot (grow: at least `rows`), else a new one."""
        dtypes = tuple(_frame_dtype(a) for a in srcs[:2])
        if isinstance(ring, cls) and ring.key[2:] == (dtypes, device, slots) and (ring.rows == rows or (grow and ring.rows > rows)):
            return ring
        return cls(rows, dtypes, device, slots)

    @property
    def pinned_bytes(self):
        return sum(t.numel() * t.element_size() for slot in self.pin for t in slot)

    def _tables(self, bufs, rows=None):
        """(offset [2,rows] int64, window [2,rows,4] int32, valid [2,rows] int32) carved out of a slot's table buffer."""
        r, tab = self.rows, bufs[4]
        off, win, val = tab[: 16 * r].view(torch.int64).view(2, r), tab[16 * r: 48 * r].view(torch.int32).view(2, r, 4), tab[48 * r:].view(torch.int32).view(2, r)
        return (off, win, val) if rows is None else (off[:, :rows], win[:, :rows], val[:, :rows])

    def wait(self, slot):
        if self.used[slot] and self.h2d[slot] is not None:
            self.h2d[slot].synchronize()                   # the copy that last read this slot's pinned buffers has finished

    def stage(self, slot, srcs, lo, hi, kinds=None, parts=None):
        """Host threads: the crop windows of poses [lo, hi) of (rgb1, rgb2, mask1, mask2) into the slot's pinned buffers (after `wait`)."""
        pool, n = _host_pool(), hi - lo
        assert 0 < n <= self.rows
        masks = []
        for v in (0, 1):
            m = srcs[2 + v]
            if m.dtype in (np.uint8, np.bool_):
                masks.append((m, lo))
                continue
            if self._mask_bytes is None or self._mask_bytes.shape[2:] != m.shape[1:]:
                self._mask_bytes = np.empty((2, self.rows) + tuple(m.shape[1:]), dtype=np.uint8)
            masks.append((self._mask_bytes[v], 0))
        for f in [f for v in (0, 1) if masks[v][0] is not srcs[2 + v] for f in stage_rows(self._mask_bytes[v], srcs[2 + v], lo, hi, "mask", pool, parts)]:
            f.result()
        off_t, win_t, val_t = (t.numpy() for t in self._tables(self.pin[slot]))
        totals, futs = [], []
        found = [mask_windows_pooled(m[m0: m0 + n], pool) for m, m0 in masks]        # both views' windows are looked for at once
        for v in (0, 1):
            m, m0 = masks[v]
            win_t[v, :n], val_t[v, :n] = gather_windows(found[v])
            off_t[v, :n], tot = window_offsets(win_t[v, :n])
            totals.append(tot)
            futs += pack_windows(self.host[slot][v], self.host[slot][2 + v], srcs[v][lo:hi], m[m0: m0 + n], 0, n, win_t[v], off_t[v], pool)
        for f in futs:
            f.result()
        self.totals[slot] = tuple(totals)
        self.shape[slot] = tuple(srcs[0].shape[1:3])

    def copy(self, slot, rows):
        """Start the copy of the slot's used prefixes on the current stream and record its event; returns the slot's `PackedViews`."""
        pin, dev = self.pin[slot], self.dev[slot]
        for v in (0, 1):
            tot = self.totals[slot][v]
            dev[v][: 3 * tot].copy_(pin[v][: 3 * tot], non_blocking=True)
            dev[2 + v][:tot].copy_(pin[2 + v][:tot], non_blocking=True)
            self.payload_bytes += tot * (3 * pin[v].element_size() + 1)
        dev[4].copy_(pin[4], non_blocking=True)
        self.table_bytes += pin[4].numel()
        if self.h2d[slot] is not None:
            self.h2d[slot].record()
        self.used[slot] = True
        off, win, val = self._tables(dev, rows)
        H, W = self.shape[slot]
        return PackedViews(dev[:2], dev[2:4], off, win, val, H, W)


def frames_payload_bytes(rgb1, rgb2, mask1, mask2):
    """Bytes the whole-frame upload hands to the copy engine for these arrays: frames cross as float32 (uint8: as bytes), masks as one
    byte per pixel; an array that already is a CUDA tensor is not uploaded.  For [n,H,W,3] host frames of one kind: 2 n H W (3 px_bytes + 1)."""
    total = 0
    for i, x in enumerate((rgb1, rgb2, mask1, mask2)):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            continue
        first = x if hasattr(x, "dtype") else x[0]
        count = int(np.prod(np.shape(x))) if hasattr(x, "shape") else len(x) * int(np.prod(np.shape(first)))
        total += count * (1 if i >= 2 or str(getattr(first, "dtype", "")).endswith("uint8") else 4)
    return total


class _Trace:
    """Per-chunk timings of the pipeline for RGBM_UPLOAD_TRACE=1 (tools/boundary_trace.py); every method does nothing when it is off."""

    def __init__(self):
        self.rows = [] if os.environ.get("RGBM_UPLOAD_TRACE") == "1" else None

    def begin(self):                                       # a chunk's loop iteration starts
        if self.rows is not None:
            self.t0 = self.t = time.perf_counter()
            self.rows.append([[torch.cuda.Event(enable_timing=True) for _ in range(4)]])

    def lap(self, since_begin=False):                      # host ms since the previous lap (or since begin)
        if self.rows is not None:
            now = time.perf_counter()
            self.rows[-1].append(round((now - (self.t0 if since_begin else self.t)) * 1e3, 2))
            self.t = now

    def mark(self, c, i, stream):                          # device clock i of chunk c: copy start, copy end, kernels start, kernels end
        if self.rows is not None:
            self.rows[c][0][i].record(stream)

    def report(self, upload_bytes=None):
        """After the device has finished the call.  upload_bytes: the call's payload handed to the copy engine (upload_bytes_last_call)."""
        if self.rows is not None:
            e00 = self.rows[0][0][0]
            rows = [(w, st, tot) + tuple(round(e00.elapsed_time(e), 1) for e in ev) for (ev, w, st, tot) in self.rows]
            print("[rgbm upload trace] per chunk (host: wait for slot ms, stage ms, whole iteration ms | device clock from the first copy's start: copy start, "
                  "copy end, kernels start, kernels end):", rows, *(() if upload_bytes is None else ("upload bytes:", int(upload_bytes))), file=sys.stderr)


class ChunkPipeline:
    """`estimate` with `hip_prepare: device` for host arrays (what rl_pose.py:210-218 hands over: [N,480,640,3] float64 frames,
    3.8 GB per call at N = 256).  Batches larger than `hip_upload_chunk` poses (default 32: measured best of 8 .. 128 for float64 and
    float32 frames in bf16 and bf16x3, tools/boundary_chunks.py; 1 GB of pinned staging for float64 frames) run as a three-stage pipeline over
    chunks of poses: host threads copy chunk c + 1 into pinned staging buffers while the copy engine moves chunk c to the device
    on its own stream and the kernels (dtype conversion, crop / resize / subset, network, post-processing) work on chunk c - 1.
    Poses are independent, but a chunk is a smaller batch: below ~1000 GEMM rows per launch and at launches that fit one round of the
    persistent grid the dispatcher picks other tiles (summation order), so a pose's box agrees with the unchunked call's to the
    storage type's rounding (1e-6 .. 1e-5 relative in fp32 / bf16x3), not bit for bit (include/rgbm.h, rgbm_set_tuning).

    Two events per slot keep a buffer from being overwritten while it is read: `ring.h2d[slot]` (the copy out of the pinned buffers has
    finished) and `done[slot]` (the kernels that read the device buffers have finished)."""

    def __init__(self, ring):
        self.ring, self.chunk, self.device = ring, ring.rows, ring.device
        self.done = [torch.cuda.Event(), torch.cuda.Event()]
        self.stream = torch.cuda.Stream(device=self.device)
        self.trace = _Trace()

    @classmethod
    def matching(cls, pipe, chunk, srcs, device, windows=False):
        """`pipe` if it was built for these host arrays (rgb1, rgb2, mask1, mask2), this chunk size and this kind of upload (windows: a
        `WindowRing`, whose slots hold the packed crop windows of a chunk and whose `copy` returns `PackedViews`), else a new one."""
        if windows:
            ring = WindowRing.matching(pipe and pipe.ring, chunk, srcs, device)
        else:
            dtypes = [_frame_dtype(a) for a in srcs[:2]] + [torch.uint8, torch.uint8]
            ring = StagingRing.matching(pipe and pipe.ring, chunk, [a.shape[1:] for a in srcs], dtypes, device)
        return pipe if pipe is not None and ring is pipe.ring else cls(ring)

    def _load(self, srcs, c, a, b, after_done):
        """Stage poses [a, b) into slot c & 1 and start its copy on the upload stream; returns the slot's device rows (a `WindowRing`: the
        slot's `PackedViews` — the ring decides what is staged and copied, the schedule is the same)."""
        slot, tr = c & 1, self.trace
        reused = self.ring.used[slot]
        tr.begin()
        self.ring.wait(slot)
        tr.lap()
        self.ring.stage(slot, srcs, a, b, ("frame", "frame", "mask", "mask"), max(1, _HOST_THREADS // 2))      # overlaps the device's work on the previous chunks
        tr.lap()
        with torch.cuda.stream(self.stream):
            if reused and after_done:
                self.stream.wait_event(self.done[slot])    # the kernels that read this slot's device buffers are done
            tr.mark(c, 0, self.stream)
            d = self.ring.copy(slot, b - a)
            tr.mark(c, 1, self.stream)
        return d

    def run(self, srcs, n, network):
        """network(a, b, d): enqueue everything for poses [a, b) on the current stream, reading the device rows d."""
        cur = torch.cuda.current_stream(self.device)
        tr = self.trace = _Trace()
        for c, a in enumerate(range(0, n, self.chunk)):
            b = min(a + self.chunk, n)
            d = self._load(srcs, c, a, b, after_done=True)
            cur.wait_event(self.ring.h2d[c & 1])
            tr.mark(c, 2, cur)
            network(a, b, d)
            self.done[c & 1].record(cur)
            tr.mark(c, 3, cur)
            tr.lap(since_begin=True)

    def run_keyed(self, srcs, n, prepare, network):
        """The schedule of hip_feature_cache: "content".  The network of a chunk cannot be enqueued before the chunk's keys are on the
        host, and a wait for them on the kernels' stream would also wait for the previous chunk's network (staging, copy and kernels
        back to back again).  So the crop preparation and the fingerprint of chunk c run on the upload stream behind that chunk's copy
        (`prepare(a, b, d)` -> pending), and its network (`network(pending)`, current stream) is enqueued one loop iteration later,
        after chunk c + 1 has been staged and its copy started: by then the keys have long arrived.  No `done` wait: the upload
        stream's own preparation reads the device rows, in order."""
        cur = torch.cuda.current_stream(self.device)
        tr = self.trace = _Trace()
        consts = torch.cuda.Event()
        consts.record(cur)                                 # what the caller wrote on this stream (K), the upload stream's preparation reads
        self.stream.wait_event(consts)
        pending = None

        def finish(pc, p):
            tr.mark(pc, 2, cur)
            network(p)
            tr.mark(pc, 3, cur)
        for c, a in enumerate(range(0, n, self.chunk)):
            b = min(a + self.chunk, n)
            d = self._load(srcs, c, a, b, after_done=False)
            with torch.cuda.stream(self.stream):
                nxt = prepare(a, b, d)
            if pending is not None:
                finish(*pending)
            pending = (c, nxt)
            tr.lap(since_begin=True)
        if pending is not None:
            finish(*pending)

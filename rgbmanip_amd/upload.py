"""Host frames and masks -> HBM: the conversion on the way into pinned staging (`stage_rows`), the double-buffered staging ring, the
whole-array uploads (`frames_to_device` / `masks_to_device`) and the chunk pipeline of `estimate()` (`ChunkPipeline`)."""
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

    def report(self):
        """After the device has finished the call."""
        if self.rows is not None:
            e00 = self.rows[0][0][0]
            rows = [(w, st, tot) + tuple(round(e00.elapsed_time(e), 1) for e in ev) for (ev, w, st, tot) in self.rows]
            print("[rgbm upload trace] per chunk (host: wait for slot ms, stage ms, whole iteration ms | device clock from the first copy's start: copy start, "
                  "copy end, kernels start, kernels end):", rows, file=sys.stderr)


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
        self.ring, self.chunk, self.device = ring, ring.key[0], ring.key[3]
        self.done = [torch.cuda.Event(), torch.cuda.Event()]
        self.stream = torch.cuda.Stream(device=self.device)
        self.trace = _Trace()

    @classmethod
    def matching(cls, pipe, chunk, srcs, device):
        """`pipe` if it was built for these host arrays (rgb1, rgb2, mask1, mask2) and this chunk size, else a new one."""
        dtypes = [_frame_dtype(a) for a in srcs[:2]] + [torch.uint8, torch.uint8]
        ring = StagingRing.matching(pipe and pipe.ring, chunk, [a.shape[1:] for a in srcs], dtypes, device)
        return pipe if pipe is not None and ring is pipe.ring else cls(ring)

    def _load(self, srcs, c, a, b, after_done):
        """Stage poses [a, b) into slot c & 1 and start its copy on the upload stream; returns the slot's device rows."""
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

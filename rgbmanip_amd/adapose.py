"""Host-side wrapper of the HIP AdaPose network (the C ABI in include/rgbm.h).

`AdaPoseNet` mirrors the call surface of the reference module `StereoPoseNet_with_depth`
(`/root/reference/models/pose_estimator/AdaPose/lib/network_v5.py:301-519`): it is built from a
state_dict with the reference's key names (optionally `module.`-prefixed, as saved by the
reference's DataParallel wrapper, `interface_v5.py:48,55-56`) and called with
`(view1_img, view1_choose, view2_img, view2_choose, view1_proj, view2_proj, depth_values)`,
returning the same 10-entry dict of tensors.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .cloud import (cloud_gather, cloud_gather_views, cloud_pack, cloud_pack_views, cloud_similarity, cloud_similarity_ref,      # noqa: F401  (part of this module's surface)
                    depth_consistency, depth_consistency_ref, depth_fusion, depth_fusion_ref, depth_to_points, depth_to_points_ref)
from .verify import box_silhouette, box_silhouette_ref, cloud_in_box, cloud_in_box_ref      # noqa: F401  (likewise)

_DTYPES = {"fp32": _lib.F32, "f32": _lib.F32, "float32": _lib.F32, "bf16": _lib.BF16, "bfloat16": _lib.BF16,
           "fp16": _lib.F16, "f16": _lib.F16, "float16": _lib.F16, "bf16x3": _lib.BF16X3}


class AdaPoseNet:
    _h = None                                            # the C handle; None until rgbm_adapose_create has run (close / __del__ read it)

    def __init__(self, state_dict, dtype: str = "fp32", device: int = 0, max_chunk_views: int | None = None,
                 cost_impl: int | None = None, sparse_tail: int | None = None, options: dict | None = None,
                 norm_mode: int | str = 0, poison_workspace: bool = False, graph: bool = False, graph_max_batch: int = 32,
                 split_streams: bool | int = False, split_min_batch: int = 128, dropout: float = 0.0, dropout_seed: int = 0,
                 arch: str = "v5", regress_pose: bool = True):
        self.lib = _lib.load()
        # arch "baseline": the reference's StereoPoseNet_with_depth_baseline (lib/network_baseline.py:523-669) from its state dict - v5's
        # PSPNet and point heads, the cost volume replaced by the cross-view attention stack and depth_head.
        # regress_pose=False (baseline only): no pose branch; forward returns the reference's four keys.  hipGraph replay, Dropout2d,
        # per-sample BatchNorm3d, the dense maps and the feature cache are not implemented for it.
        # arch "realworld": the reference's StereoPoseNet_with_depth_for_realdemo (lib/network_realworld.py) from its state dict - v5 on a
        # variance cost volume, the pose rows from camera points.  forward() needs coor1= / coor2=.  dtype fp16,
        # hipGraph replay, Dropout2d, per-sample BatchNorm3d, the dense maps, forward_samples and the feature cache are refused.
        # arch "v2": the reference's StereoPoseNet (lib/network_v2.py) from its state dict - v5's PSPNet and NOCS branch, the pointwise stereo
        # part and pose_mlp1 evaluated at the chosen pixels by one kernel, a size branch and no depth / rotation / translation (DESIGN.md
        # section 5s): forward() returns view*_nocs and view*_s, the other six outputs are NaN.  All four dtypes; hipGraph replay, Dropout2d,
        # per-sample BatchNorm3d, split_streams, the dense maps, forward_samples and the feature cache are refused.
        # arch "v1": the reference's StereoPoseNet (lib/network.py) from its state dict - v2's pointwise stereo part with a 32-channel
        # fuse_conv whose result is a residual on the feature row (stage A, one kernel at the chosen pixels), v5's NOCS branch on those rows
        # (stage B) and v5's pose branch on 128-channel rows: forward() returns nocs, r, t, s of both views, the
        # depth outputs are NaN.  The refusals are those of arch "v2".
        if arch not in ("v5", "baseline", "realworld", "v2", "v1"):
            raise ValueError(f"arch must be 'v5', 'baseline', 'realworld', 'v2' or 'v1', got {arch!r}")
        self.arch = arch
        self.regress_pose = bool(regress_pose)
        if arch == "baseline":
            for key, on in (("graph", graph), ("dropout", dropout), ("norm_mode", norm_mode not in (0, "eval")), ("cost_impl", cost_impl is not None),
                            ("sparse_tail", sparse_tail is not None)):
                if on:
                    raise _lib.RgbmError(f"AdaPoseNet(arch='baseline'): {key} is not implemented for the baseline network")
        elif not regress_pose:
            raise ValueError("regress_pose=False exists for arch='baseline' only")
        if arch == "realworld":
            for key, on in (("graph", graph), ("dropout", dropout), ("norm_mode", norm_mode not in (0, "eval")), ("split_streams", split_streams),
                            ("dtype fp16", _DTYPES[dtype] == _lib.F16)):
                if on:
                    raise _lib.RgbmError(f"AdaPoseNet(arch='realworld'): {key} is not implemented for the real-world network")
        if arch in ("v2", "v1"):
            for key, on in (("graph", graph), ("dropout", dropout), ("norm_mode", norm_mode not in (0, "eval")), ("split_streams", split_streams),
                            ("cost_impl", cost_impl is not None), ("sparse_tail", sparse_tail is not None)):
                if on:
                    raise _lib.RgbmError(f"AdaPoseNet(arch='{arch}'): {key} is not implemented for the {arch} network")
        # graph: forwards of at most `graph_max_batch` poses are replayed from a hipGraph captured per batch size
        # (rgbm_adapose_forward_graph): static input / output / workspace buffers per batch size, one hipGraphLaunch instead of ~150
        # launches — the small-batch deployment path (interface_v5.py:213-227 calls the network per env; cfg/task/open_cabinet.yaml
        # ships num_envs: 8).  Larger batches run eagerly: they are bound by the kernels, not by their launches.
        self.graph = bool(graph)
        self.graph_max_batch = int(graph_max_batch)
        self._static = {}
        self._gstream = None
        self.last_graph_nodes = 0
        self._last_graph = False
        # debug: fill the whole workspace with 0xFF bytes (NaN in every storage type, -1 in index lists) in front of EVERY forward, so
        # that a kernel reading a tile the sparse cost regularisation skipped — or anything else a forward did not write itself —
        # cannot find a previous run's (correct) values there (tests/test_gpu_at_batch.py, bench.py's at-batch check)
        self.poison_workspace = bool(poison_workspace)
        # split_streams (opt-in): a forward of at least `split_min_batch` (even) poses runs as two half batches on two side streams, each with
        # its own workspace: the tail of every launch of one half (partial last round of workgroups, the drain of a persistent kernel) is
        # filled by the other half's kernels (-0.7 % bf16, -2.6 % bf16x3 at batch 256).  Same kernels, same per-pose arithmetic:
        # outputs bit-identical to the one-stream forward (tests/test_gpu_at_batch.py) — which needs a library without packed fp32
        # instructions (build.sh).  Intermediate taps (fetch) refer to the one-stream workspace and are refused after a split forward.
        # split_streams = n > 2 (round 6): n equal parts on n side streams.
        self.split_streams = bool(split_streams)
        self.split_parts = 2 if split_streams is True else max(int(split_streams), 2)
        self.split_min_batch = int(split_min_batch)
        self._split = None                           # ([side streams], [workspaces], batch)
        self._last_split = False
        if not torch.cuda.is_available():
            raise _lib.RgbmError("AdaPoseNet needs a HIP device (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.device("cuda", device)
        self.dtype_name = dtype
        self.dtype = _DTYPES[dtype]
        keep, descs = [], []
        for k, v in state_dict.items():
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if a.dtype != np.float32:
                if a.dtype.kind != "f":
                    continue                      # num_batches_tracked (int64)
                a = a.astype(np.float32)
            a = np.ascontiguousarray(a)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape) if a.ndim else (C.c_int64 * 1)(1)
            name = k.encode()
            keep.append((a, shape, name))
            descs.append(_lib.WeightDesc(name, a.ctypes.data, a.ndim, shape))
        arr = (_lib.WeightDesc * len(descs))(*descs)
        self._h = C.c_void_p()
        # norm_mode: 0 / "eval" = BatchNorm3d with running statistics (default); 1 / "per_sample" = the reference's as-shipped
        # train-mode statistics at batch 1 (every view normalised with its own volume's mean / variance)
        self.norm_mode = {"eval": 0, "per_sample": 1}.get(norm_mode, norm_mode)
        if arch == "baseline":
            _lib.check(self.lib.rgbm_adapose_create_baseline(C.byref(self._h), device, arr, len(descs), self.dtype, int(self.regress_pose)),
                       "rgbm_adapose_create_baseline")
        elif arch == "realworld":
            _lib.check(self.lib.rgbm_adapose_create_realworld(C.byref(self._h), device, arr, len(descs), self.dtype), "rgbm_adapose_create_realworld")
        elif arch == "v2":
            _lib.check(self.lib.rgbm_adapose_create_v2(C.byref(self._h), device, arr, len(descs), self.dtype), "rgbm_adapose_create_v2")
        elif arch == "v1":
            _lib.check(self.lib.rgbm_adapose_create_v1(C.byref(self._h), device, arr, len(descs), self.dtype), "rgbm_adapose_create_v1")
        else:
            _lib.check(self.lib.rgbm_adapose_create(C.byref(self._h), device, arr, len(descs), self.dtype, int(self.norm_mode)),
                       "rgbm_adapose_create")
        if max_chunk_views:
            _lib.check(self.lib.rgbm_adapose_set_chunk(self._h, int(max_chunk_views)), "rgbm_adapose_set_chunk")
        if cost_impl is not None:
            _lib.check(self.lib.rgbm_adapose_set_option(self._h, b"cost_impl", int(cost_impl)), "rgbm_adapose_set_option")
        if sparse_tail is not None:
            _lib.check(self.lib.rgbm_adapose_set_option(self._h, b"sparse_tail", int(sparse_tail)), "rgbm_adapose_set_option")
        self.options = {}                                 # what was set through this object (a sharing estimator reads view2_heads back)
        for key, val in (options or {}).items():          # any rgbm_adapose_set_option key (include/rgbm.h), e.g. fuse_final
            _lib.check(self.lib.rgbm_adapose_set_option(self._h, key.encode(), int(val)), "rgbm_adapose_set_option")
            self.options[key] = int(val)
        self._ws = None
        self._ws_B = None
        # dropout: PSPNet's Dropout2d as the reference runs it as shipped (never .eval()): seeded masks, fresh on every forward
        # (rgbm_adapose_set_dropout; 0 = off)
        self.dropout, self.dropout_seed = 0.0, 0
        self._drop_explicit = False
        if dropout:
            self.set_dropout(dropout, dropout_seed)

    # ------------------------------------------------------------------
    def set_dropout(self, p: float, seed: int = 0):
        """Turn PSPNet's Dropout2d on (0 < p < 1) or off (p = 0) and restart its mask sequence at pose 0 of `seed`.
        Synchronises the device."""
        p = float(p)
        if not (p == 0.0 or 0.0 < p < 1.0):
            raise ValueError(f"dropout p must be 0 (off) or lie in (0, 1), got {p}")
        _lib.check(self.lib.rgbm_adapose_set_dropout(self._h, p, int(seed) & (2 ** 64 - 1)), "rgbm_adapose_set_dropout")
        self.dropout, self.dropout_seed = p, int(seed)

    def dropout_masks(self, B: int) -> torch.Tensor:
        """The Dropout2d factors the last forward (batch B) used: [2B, 320] fp32 — rows: the view-1 crops, then the view-2 crops;
        columns: up_1's 256 channels, then up_2's 64.  Synchronises the device."""
        out = torch.empty(2 * B, 320, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.rgbm_adapose_dropout_masks(self._h, int(B), _lib.ptr(out)), "rgbm_adapose_dropout_masks")
        return out

    def set_dropout_masks(self, masks):
        """Explicit factors ([2B, 320], layout of `dropout_masks`) for the next forward of batch B, used instead of drawn ones (and
        the mask sequence does not advance).  Synchronises the device."""
        t = self._prep(masks, torch.float32)
        if t.dim() != 2 or t.shape[1] != 320 or t.shape[0] % 2:
            raise ValueError(f"dropout masks must be [2B, 320], got {tuple(t.shape)}")
        torch.cuda.synchronize(self.device)
        _lib.check(self.lib.rgbm_adapose_set_dropout_masks(self._h, t.shape[0] // 2, _lib.ptr(t)), "rgbm_adapose_set_dropout_masks")
        self._drop_explicit = True

    def close(self):
        if self._h is not None and self._h.value:
            self.lib.rgbm_adapose_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def workspace_bytes(self, B: int) -> int:
        n = C.c_size_t()
        _lib.check(self.lib.rgbm_adapose_workspace_bytes(self._h, B, C.byref(n)), "rgbm_adapose_workspace_bytes")
        return n.value

    def _workspace(self, B: int):
        if self._ws is None or self._ws_B != B:
            self._ws = None
            self._ws = torch.empty(self.workspace_bytes(B) + 256, dtype=torch.uint8, device=self.device)
            self._ws_B = B
        return self._aligned(self._ws)

    def _prep(self, t, dtype):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _empty_outputs(self, B):
        """The ten outputs of the reference network (network_v5.py:301-519), uninitialised."""
        shapes = {"nocs": (B, 1024, 3), "depth": (B, 1024), "r": (B, 3, 3), "t": (B, 3), "s": (B, 3)}
        return {f"view{v}_{k}": torch.empty(*shp, dtype=torch.float32, device=self.device) for k, shp in shapes.items() for v in (1, 2)}

    @staticmethod
    def _aligned(ws):
        """(256-byte aligned pointer into the workspace tensor, bytes behind it)"""
        off = (-ws.data_ptr()) % 256
        return ws.data_ptr() + off, ws.numel() - off

    def _poison(self, ws, stream=None):
        """poison_workspace: 0xFF bytes over `ws` on the stream the forward runs on (None: the current one)."""
        if self.poison_workspace:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                ws.fill_(0xFF)

    def _forward_graph(self, args):
        """Replay (first call per batch size: capture) the forward on static buffers; returns fresh output tensors."""
        def as_t(x):
            return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        args = [as_t(a) for a in args]
        B = int(args[0].shape[0])
        st = self._static.get(B)
        if st is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            i32 = dict(dtype=torch.int32, device=self.device)
            ins = [torch.empty(B, 3, 224, 224, **f32), torch.empty(B, 1024, **i32), torch.empty(B, 3, 224, 224, **f32), torch.empty(B, 1024, **i32),
                   torch.empty(B, 4, 4, **f32), torch.empty(B, 4, 4, **f32), torch.empty(B, 24, **f32)]
            out = self._empty_outputs(B)
            ws = torch.empty(self.workspace_bytes(B) + 256, dtype=torch.uint8, device=self.device)
            st = self._static[B] = (ins, out, ws)
        ins, out, ws = st
        self._drop_explicit = False
        for dst, src in zip(ins, args):
            assert tuple(src.shape) == tuple(dst.shape), (tuple(src.shape), tuple(dst.shape))
            dst.copy_(src, non_blocking=True)              # converts dtype / uploads as needed, on the caller's stream
        if self._gstream is None:
            self._gstream = torch.cuda.Stream(device=self.device)      # capture is not allowed on the default stream
        cur = torch.cuda.current_stream(self.device)
        gs = self._gstream
        gs.wait_stream(cur)
        ws_ptr, ws_bytes = self._aligned(ws)
        o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
        nodes, cap = C.c_int32(), C.c_int32()
        self._poison(ws, gs)
        # (img1, choose1, img2, choose2, P1, P2, depths) -> the C ABI's (img1, img2, choose1, choose2, P1, P2, depths)
        _lib.check(self.lib.rgbm_adapose_forward_graph(self._h, B, _lib.ptr(ins[0]), _lib.ptr(ins[2]), _lib.ptr(ins[1]), _lib.ptr(ins[3]),
                                                       _lib.ptr(ins[4]), _lib.ptr(ins[5]), _lib.ptr(ins[6]), C.c_void_p(ws_ptr),
                                                       ws_bytes, C.byref(o), C.c_void_p(gs.cuda_stream), C.byref(nodes), C.byref(cap)),
                   "rgbm_adapose_forward_graph")
        self.last_graph_nodes = nodes.value
        cur.wait_stream(gs)
        return {k: v.clone() for k, v in out.items()}      # the static outputs are overwritten by the next replay

    def forward(self, view1_img, view1_choose, view2_img, view2_choose, view1_proj, view2_proj, depth_values,
                stop_after: int = 0, stream=None, dense_depth: bool = False, dense_nocs: bool = False, coor1=None, coor2=None):
        """The reference network's call.  `dense_depth=True` (rgbm_adapose_forward_dense): the same dict plus `view1_depth_map` /
        `view1_depth_conf` and, with the view-2 heads, `view2_depth_map` / `view2_depth_conf` — [B, 224, 224] float32 each: the expected
        depth and the largest probability over the 24 planes at every pixel of the crop.  That call runs the dense cost regularisation
        and the dense tail whatever the net's options say (and leaves them as they are), always eagerly on one stream.
        `dense_nocs=True` (rgbm_adapose_forward_maps), alone or with `dense_depth`: plus `view1_nocs_map` (and `view2_nocs_map` with the
        view-2 heads) [B, 224, 224, 3] float32, the NOCS branch at every pixel; the map read at `choose` is `view*_nocs` bit for bit.
        Alone it leaves the ten outputs those of the plain forward (the net's own options, eagerly on one stream).
        `coor1=` / `coor2=` [B, 1024, 2] float32 (arch "realworld" only, required there): the chosen points' pixel coordinates divided by
        the frame's width and height, the reference network's view1_pts2d / view2_pts2d arguments (network_realworld.py:133)."""
        if self.arch == "realworld":
            if dense_depth or dense_nocs:
                raise _lib.RgbmError("AdaPoseNet(arch='realworld'): dense_depth / dense_nocs are not implemented for the real-world network")
            if coor1 is None or coor2 is None:
                raise _lib.RgbmError("AdaPoseNet(arch='realworld'): forward needs coor1= and coor2= (the normalised point coordinates)")
        elif coor1 is not None or coor2 is not None:
            raise _lib.RgbmError("coor1 / coor2 are inputs of arch='realworld' only")
        if self.arch in ("v2", "v1") and (dense_depth or dense_nocs):
            raise _lib.RgbmError(f"AdaPoseNet(arch='{self.arch}'): dense_depth / dense_nocs are not implemented for the {self.arch} network")
        if dense_depth or dense_nocs:
            assert stop_after == 0, "dense_depth / dense_nocs: the whole forward"
            return self._forward_dense((view1_img, view2_img, view1_choose, view2_choose, view1_proj, view2_proj, depth_values), stream,
                                       depth=bool(dense_depth), nocs=bool(dense_nocs))
        if self.graph and stop_after == 0 and stream is None and len(view1_img) <= self.graph_max_batch:
            self._last_graph = True
            return self._forward_graph((view1_img, view1_choose, view2_img, view2_choose, view1_proj, view2_proj, depth_values))
        self._last_graph = False
        img1 = self._prep(view1_img, torch.float32)
        img2 = self._prep(view2_img, torch.float32)
        ch1 = self._prep(view1_choose, torch.int32)
        ch2 = self._prep(view2_choose, torch.int32)
        P1 = self._prep(view1_proj, torch.float32)
        P2 = self._prep(view2_proj, torch.float32)
        dep = self._prep(depth_values, torch.float32)
        B = img1.shape[0]
        assert img1.shape == (B, 3, 224, 224) and img2.shape == img1.shape, img1.shape
        assert ch1.shape == (B, 1024) and ch2.shape == ch1.shape
        assert P1.shape == (B, 4, 4) and P2.shape == (B, 4, 4) and dep.shape == (B, 24)
        out = self._empty_outputs(B)
        # with dropout the parts would share the handle's pose counter and factor buffer (rgbm.h): the forward runs on one stream (the
        # split forward computes the same outputs)
        if self.split_streams and stop_after == 0 and B >= self.split_min_batch and B % self.split_parts == 0 and not self.dropout \
                and not self._drop_explicit:
            self._forward_split(B, (img1, img2, ch1, ch2, P1, P2, dep), out, stream)
            return out
        self._last_split = False
        self._drop_explicit = False
        o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
        ws_ptr, ws_bytes = self._workspace(B)
        self._poison(self._ws, stream)
        if self.arch == "realworld":
            c1 = self._prep(coor1, torch.float32)
            c2 = self._prep(coor2, torch.float32)
            assert c1.shape == (B, 1024, 2) and c2.shape == c1.shape, c1.shape
            _lib.check(self.lib.rgbm_adapose_forward_realworld(self._h, B, _lib.ptr(img1), _lib.ptr(img2), _lib.ptr(ch1), _lib.ptr(ch2),
                                                               _lib.ptr(c1), _lib.ptr(c2), _lib.ptr(P1), _lib.ptr(P2), _lib.ptr(dep),
                                                               C.c_void_p(ws_ptr), ws_bytes, C.byref(o), stop_after, _lib.stream_ptr(stream)),
                       "rgbm_adapose_forward_realworld")
            self._last = (img1, img2, ch1, ch2, P1, P2, dep, c1, c2)
            return out
        _lib.check(self.lib.rgbm_adapose_forward_ex(self._h, B, _lib.ptr(img1), _lib.ptr(img2), _lib.ptr(ch1), _lib.ptr(ch2),
                                                    _lib.ptr(P1), _lib.ptr(P2), _lib.ptr(dep), C.c_void_p(ws_ptr), ws_bytes,
                                                    C.byref(o), stop_after, _lib.stream_ptr(stream)), "rgbm_adapose_forward")
        self._last = (img1, img2, ch1, ch2, P1, P2, dep)     # keep inputs alive until the stream has consumed them
        if self.arch == "baseline" and not self.regress_pose:      # the reference's four keys (network_baseline.py:667-670)
            return {k: out[k] for k in ("view1_nocs", "view2_nocs", "view1_depth", "view2_depth")}
        return out

    def samples_workspace_bytes(self, B: int, samples: int) -> int:
        n = C.c_size_t()
        _lib.check(self.lib.rgbm_adapose_samples_workspace_bytes(self._h, int(B), int(samples), C.byref(n)), "rgbm_adapose_samples_workspace_bytes")
        return n.value

    def forward_samples(self, view1_img, view1_choose, view2_img, view2_choose, view1_proj, view2_proj, depth_values, samples: int,
                        stream=None):
        """`samples` Dropout2d draws of every pose from one pass over the backbone in front of the first Dropout2d site
        (rgbm_adapose_forward_samples): the arguments of `forward` for B poses -> the ten `OUT_KEYS` of `forward`, shaped
        [samples, B, ...].  Sample s of pose b is pose s * B + b of a plain `forward` of the B poses tiled `samples` times - the masks of
        global poses counter + s * B + b, the counter advanced by samples * B, `dropout_masks(samples * B)` and `set_dropout_masks` for
        samples * B poses as there.  Needs Dropout2d on (`set_dropout`) or masks loaded; refused for arch "baseline".  Always eager and
        on one stream, like every forward with dropout; no graph, split, dense or cached form."""
        S = int(samples)
        dts = (torch.float32, torch.float32, torch.int32, torch.int32, torch.float32, torch.float32, torch.float32)
        args = (view1_img, view2_img, view1_choose, view2_choose, view1_proj, view2_proj, depth_values)
        img1, img2, ch1, ch2, P1, P2, dep = t = tuple(self._prep(a, d) for a, d in zip(args, dts))
        B = img1.shape[0]
        assert img1.shape == (B, 3, 224, 224) and img2.shape == img1.shape, img1.shape
        assert ch1.shape == (B, 1024) and ch2.shape == ch1.shape
        assert P1.shape == (B, 4, 4) and P2.shape == (B, 4, 4) and dep.shape == (B, 24)
        out = self._empty_outputs(max(S, 1) * B)
        o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
        ws_ptr, ws_bytes = self._workspace_at_least(self.samples_workspace_bytes(B, S))      # refuses S < 1 and the baseline network
        self._poison(self._ws, stream)
        _lib.check(self.lib.rgbm_adapose_forward_samples(self._h, B, S, *[_lib.ptr(x) for x in t], C.c_void_p(ws_ptr), ws_bytes, C.byref(o),
                                                         _lib.stream_ptr(stream)), "rgbm_adapose_forward_samples")
        self._drop_explicit = False
        self._last_split = self._last_graph = False
        self._last = t                                        # keep inputs alive until the stream has consumed them
        return {k: v.view(S, B, *v.shape[1:]) for k, v in out.items()}

    def view_fusion(self, x1, x2, stream=None):
        """The attention stack alone (rgbm_view_fusion) with this net's weights: rows x1 / x2 [B, P, 32] (point-major; read as float32),
        P a multiple of 32 in [32, 4096] -> (y1, y2) [B, P, 32] float32 CUDA."""
        a = torch.as_tensor(x1).to(device=self.device, dtype=torch.float32).contiguous()
        b = torch.as_tensor(x2).to(device=self.device, dtype=torch.float32).contiguous()
        if a.dim() != 3 or a.shape[2] != 32 or b.shape != a.shape or a.shape[0] < 1 or a.shape[1] % 32 or not 32 <= a.shape[1] <= 4096:
            raise ValueError(f"view_fusion: x1 / x2 [B, P, 32] with P a multiple of 32 in [32, 4096], got {tuple(a.shape)} and {tuple(b.shape)}")
        B, P = int(a.shape[0]), int(a.shape[1])
        nb = C.c_size_t()
        _lib.check(self.lib.rgbm_view_fusion_scratch_bytes(B, P, C.byref(nb)), "rgbm_view_fusion_scratch_bytes")
        scratch = torch.empty(nb.value // 4, dtype=torch.float32, device=self.device)
        y1, y2 = torch.empty_like(a), torch.empty_like(a)
        if stream is not None:
            for t in (scratch, y1, y2, a, b):
                t.record_stream(stream)
        _lib.check(self.lib.rgbm_view_fusion(self._h, _lib.ptr(a), _lib.ptr(b), B, P, _lib.ptr(y1), _lib.ptr(y2), _lib.ptr(scratch), nb.value,
                                             _lib.stream_ptr(stream)), "rgbm_view_fusion")
        return y1, y2

    def depth_head(self, x, stream=None):
        """depth_head alone (rgbm_depth_head) with this net's weights: rows x [..., 32] -> [...] float32 CUDA."""
        t = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).contiguous()
        if t.dim() < 2 or t.shape[-1] != 32 or t.numel() == 0:
            raise ValueError(f"depth_head: x [..., 32], got {tuple(t.shape)}")
        out = torch.empty(t.shape[:-1], dtype=torch.float32, device=self.device)
        if stream is not None:
            t.record_stream(stream)
            out.record_stream(stream)
        _lib.check(self.lib.rgbm_depth_head(self._h, _lib.ptr(t), t.numel() // 32, _lib.ptr(out), _lib.stream_ptr(stream)), "rgbm_depth_head")
        return out

    def dense_workspace_bytes(self, B: int) -> int:
        n = C.c_size_t()
        _lib.check(self.lib.rgbm_adapose_dense_workspace_bytes(self._h, B, C.byref(n)), "rgbm_adapose_dense_workspace_bytes")
        return n.value

    def _forward_dense(self, args, stream, depth: bool = True, nocs: bool = False):
        dts = (torch.float32, torch.float32, torch.int32, torch.int32, torch.float32, torch.float32, torch.float32)
        img1, img2, ch1, ch2, P1, P2, dep = t = tuple(self._prep(a, d) for a, d in zip(args, dts))
        B = img1.shape[0]
        assert img1.shape == (B, 3, 224, 224) and img2.shape == img1.shape, img1.shape
        assert ch1.shape == (B, 1024) and ch2.shape == ch1.shape
        assert P1.shape == (B, 4, 4) and P2.shape == (B, 4, 4) and dep.shape == (B, 24)
        out = self._empty_outputs(B)
        views = 2 if self.options.get("view2_heads", 1) else 1
        maps = torch.empty(2, views * B, 224, 224, dtype=torch.float32, device=self.device) if depth else None      # depth, confidence
        nmap = torch.empty(views * B, 224, 224, 3, dtype=torch.float32, device=self.device) if nocs else None
        o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
        ws_ptr, ws_bytes = self._workspace_at_least(self.dense_workspace_bytes(B) if depth else self.workspace_bytes(B))       # grows on first use
        self._poison(self._ws, stream)
        self._drop_explicit = False
        if nocs:
            _lib.check(self.lib.rgbm_adapose_forward_maps(self._h, B, *[_lib.ptr(x) for x in t], C.c_void_p(ws_ptr), ws_bytes, C.byref(o),
                                                          _lib.ptr(maps[0]) if depth else None, _lib.ptr(maps[1]) if depth else None,
                                                          _lib.ptr(nmap), _lib.stream_ptr(stream)), "rgbm_adapose_forward_maps")
        else:
            _lib.check(self.lib.rgbm_adapose_forward_dense(self._h, B, *[_lib.ptr(x) for x in t], C.c_void_p(ws_ptr), ws_bytes, C.byref(o),
                                                           _lib.ptr(maps[0]), _lib.ptr(maps[1]), _lib.stream_ptr(stream)),
                       "rgbm_adapose_forward_dense")
        self._last_split = self._last_graph = False
        self._last = t                                        # keep inputs alive until the stream has consumed them
        for v in range(views):
            if depth:
                out[f"view{v + 1}_depth_map"] = maps[0, v * B:(v + 1) * B]
                out[f"view{v + 1}_depth_conf"] = maps[1, v * B:(v + 1) * B]
            if nocs:
                out[f"view{v + 1}_nocs_map"] = nmap[v * B:(v + 1) * B]
        return out

    def nocs_map(self, feat, stream=None):
        """The dense NOCS kernel alone (rgbm_nocs_map) with this net's weights: feat [V, HW, 32] (any float type; read as float32) ->
        [V, HW, 3] float32 CUDA, V * HW a multiple of 64."""
        f = torch.as_tensor(feat).to(device=self.device, dtype=torch.float32).contiguous()
        if f.dim() != 3 or f.shape[2] != 32 or f.shape[0] * f.shape[1] == 0 or (f.shape[0] * f.shape[1]) % 64:
            raise ValueError(f"nocs_map: feat [V, HW, 32] with V * HW a positive multiple of 64, got {tuple(f.shape)}")
        out = torch.empty(f.shape[0], f.shape[1], 3, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.rgbm_nocs_map(self._h, _lib.ptr(f), int(f.shape[0]), int(f.shape[1]), _lib.ptr(out), _lib.stream_ptr(stream)),
                   "rgbm_nocs_map")
        return out

    def _forward_split(self, B, args, out, stream):
        n = self.split_parts
        h = B // n
        if self._split is None or self._split[2] != B:
            self._split = None
            need = self.workspace_bytes(h) + 256
            self._split = ([torch.cuda.Stream(device=self.device) for _ in range(n)],
                           [torch.empty(need, dtype=torch.uint8, device=self.device) for _ in range(n)], B)
        side, wss, _ = self._split
        cur = stream if stream is not None else torch.cuda.current_stream(self.device)
        fork = torch.cuda.Event()
        fork.record(cur)
        for i in range(n):
            si, ws = side[i], wss[i]
            si.wait_event(fork)                       # inputs (and the previous use of the outputs) are ordered on `cur`
            ws_ptr, ws_bytes = self._aligned(ws)
            self._poison(ws, si)
            sl = slice(i * h, (i + 1) * h)
            o = _lib.AdaposeOut(*[out[n][sl].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
            a = [t[sl] for t in args]                  # leading-dimension slices of contiguous tensors: contiguous views
            _lib.check(self.lib.rgbm_adapose_forward_ex(self._h, h, *[_lib.ptr(t) for t in a], C.c_void_p(ws_ptr),
                                                        ws_bytes, C.byref(o), 0, _lib.stream_ptr(si)), "rgbm_adapose_forward")
        for si in side:
            join = torch.cuda.Event()
            join.record(si)
            cur.wait_event(join)
        self._last = args
        self._last_split = True

    __call__ = forward

    # ------------------------------------------------------------------ feature cache (include/rgbm.h: rgbm_adapose_features)
    @property
    def feature_bytes(self) -> int:
        """Size of one view's feature record with the current options: what the stages behind the PSPNet read of it."""
        n = C.c_size_t()
        _lib.check(self.lib.rgbm_adapose_feature_bytes(self._h, C.byref(n)), "rgbm_adapose_feature_bytes")
        return n.value

    def feature_pool(self, records: int) -> torch.Tensor:
        """An uninitialised pool of `records` feature records (uint8 CUDA tensor, [records, feature_bytes])."""
        return torch.empty(int(records), self.feature_bytes, dtype=torch.uint8, device=self.device)

    def _workspace_at_least(self, need: int):
        if self._ws is None or self._ws.numel() < need + 256:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            self._ws_B = None                         # sized by bytes, not by a batch: a plain forward sizes its own again
        return self._aligned(self._ws)

    def _pool_records(self, pool) -> int:
        if not (isinstance(pool, torch.Tensor) and pool.is_cuda and pool.dtype == torch.uint8 and pool.is_contiguous()):
            raise ValueError("feature pool: a contiguous uint8 CUDA tensor (AdaPoseNet.feature_pool)")
        fb = self.feature_bytes
        if pool.numel() < fb or pool.numel() % fb:
            raise ValueError(f"feature pool: {pool.numel()} bytes is not a whole number of {fb}-byte records")
        return pool.numel() // fb

    def features(self, img, slots, pool, stream=None):
        """Run the PSPNet on the V >= 1 views img [V,3,224,224] and write view v's feature record to record slots[v] of `pool`
        (a slot outside the pool is skipped on the device).  Refused with Dropout2d on."""
        img = self._prep(img, torch.float32)
        slots = self._prep(slots, torch.int32)
        V = img.shape[0]
        assert img.shape == (V, 3, 224, 224) and slots.shape == (V,), (img.shape, slots.shape)
        records = self._pool_records(pool)
        n = C.c_size_t()
        _lib.check(self.lib.rgbm_adapose_features_workspace_bytes(self._h, V, C.byref(n)), "rgbm_adapose_features_workspace_bytes")
        ws_ptr, ws_bytes = self._workspace_at_least(n.value)
        self._poison(self._ws, stream)
        _lib.check(self.lib.rgbm_adapose_features(self._h, V, _lib.ptr(img), _lib.ptr(slots), _lib.ptr(pool), records, C.c_void_p(ws_ptr),
                                                  ws_bytes, _lib.stream_ptr(stream)), "rgbm_adapose_features")
        self._last_feat = (img, slots)                    # keep inputs alive until the stream has consumed them

    def forward_cached(self, pool, slot1, slot2, view1_choose, view2_choose, view1_proj, view2_proj, depth_values, stream=None):
        """`forward` with the two crops of pose b read from feature records slot1[b] / slot2[b] of `pool` instead of computed from
        images; returns the same output dict.  A pose with a slot outside the pool gets NaN outputs.  Refused with Dropout2d on."""
        s1 = self._prep(slot1, torch.int32)
        s2 = self._prep(slot2, torch.int32)
        ch1 = self._prep(view1_choose, torch.int32)
        ch2 = self._prep(view2_choose, torch.int32)
        P1 = self._prep(view1_proj, torch.float32)
        P2 = self._prep(view2_proj, torch.float32)
        dep = self._prep(depth_values, torch.float32)
        B = ch1.shape[0]
        assert s1.shape == (B,) and s2.shape == (B,) and ch1.shape == (B, 1024) and ch2.shape == ch1.shape
        assert P1.shape == (B, 4, 4) and P2.shape == (B, 4, 4) and dep.shape == (B, 24)
        records = self._pool_records(pool)
        out = self._empty_outputs(B)
        o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
        ws_ptr, ws_bytes = self._workspace_at_least(self.workspace_bytes(B))
        self._poison(self._ws, stream)
        _lib.check(self.lib.rgbm_adapose_forward_cached(self._h, B, _lib.ptr(pool), records, _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(ch1),
                                                        _lib.ptr(ch2), _lib.ptr(P1), _lib.ptr(P2), _lib.ptr(dep), C.c_void_p(ws_ptr), ws_bytes,
                                                        C.byref(o), _lib.stream_ptr(stream)), "rgbm_adapose_forward_cached")
        self._last_split = False
        self._last_graph = False
        self._last = (s1, s2, ch1, ch2, P1, P2, dep)
        return out

    def v2_point_rows(self, feat, choose, P_views, depth_values, views: int | None = None, stream=None):
        """The per-point plane-sweep head alone with this net's weights (arch "v2"; rgbm_v2_point_rows): feat [2B, S, S, 32] float32 feature
        maps (views = the view-1 crops, then the view-2 crops), choose [views, P] pixel indices, P_views [2B, 4, 4], depth_values [B, 24]
        -> (rows [views, P, 64] = pose_mlp1's output, fuse [views, P, 64] = fuse_conv's, planes [views, P, 24] = volume_conv's)."""
        feat = self._prep(feat, torch.float32)
        ch = self._prep(choose, torch.int32)
        Pv = self._prep(P_views, torch.float32)
        dep = self._prep(depth_values, torch.float32)
        V, S = feat.shape[0], feat.shape[1]
        B = V // 2
        views = ch.shape[0] if views is None else int(views)
        P = ch.shape[1]
        assert feat.shape == (2 * B, S, S, 32) and Pv.shape == (2 * B, 4, 4) and dep.shape == (B, 24) and views in (B, 2 * B), (feat.shape, ch.shape)
        assert ch.shape == (views, P)
        homog = torch.empty(2 * B, 12, dtype=torch.float32, device=self.device)
        rows = torch.empty(views, P, 64, dtype=torch.float32, device=self.device)
        fuse = torch.empty(views, P, 64, dtype=torch.float32, device=self.device)
        planes = torch.empty(views, P, 24, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.rgbm_v2_point_rows(self._h, _lib.ptr(feat), _lib.ptr(ch), _lib.ptr(Pv), _lib.ptr(dep), _lib.ptr(homog), _lib.ptr(rows),
                                               _lib.ptr(fuse), _lib.ptr(planes), B, P, S, views, _lib.stream_ptr(stream)), "rgbm_v2_point_rows")
        self._last_v2 = (feat, ch, Pv, dep, homog)      # keep inputs alive until the stream has consumed them
        return rows, fuse, planes

    def v1_point_rows(self, feat, choose, P_views, depth_values, views: int | None = None, stream=None, stage_b: bool = True):
        """Stages A and B of the v1 heads alone with this net's weights (arch "v1"; rgbm_v1_point_rows): feat [2B, S, S, 32] float32 feature
        maps (views = the view-1 crops, then the view-2 crops), choose [views, P] pixel indices, P_views [2B, 4, 4], depth_values [B, 24]
        -> (fused [views, P, 32] = relu(feat + fuse_conv(planes)), nocs4 [views, P, 4], rows [views, P, 128] = the pose rows,
        planes [views, P, 24] = volume_conv's).  stage_b=False: stage A alone, nocs4 and rows are None."""
        feat = self._prep(feat, torch.float32)
        ch = self._prep(choose, torch.int32)
        Pv = self._prep(P_views, torch.float32)
        dep = self._prep(depth_values, torch.float32)
        V, S = feat.shape[0], feat.shape[1]
        B = V // 2
        views = ch.shape[0] if views is None else int(views)
        P = ch.shape[1]
        assert feat.shape == (2 * B, S, S, 32) and Pv.shape == (2 * B, 4, 4) and dep.shape == (B, 24) and views in (B, 2 * B), (feat.shape, ch.shape)
        assert ch.shape == (views, P)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)      # noqa: E731
        homog, fused, planes = new(2 * B, 12), new(views, P, 32), new(views, P, 24)
        nocs4, rows, scratch = (new(views, P, 4), new(views, P, 128), new(views * P * 288)) if stage_b else (None, None, None)
        _lib.check(self.lib.rgbm_v1_point_rows(self._h, _lib.ptr(feat), _lib.ptr(ch), _lib.ptr(Pv), _lib.ptr(dep), _lib.ptr(homog), _lib.ptr(fused),
                                               _lib.ptr(nocs4), _lib.ptr(rows), _lib.ptr(planes), _lib.ptr(scratch), B, P, S, views,
                                               _lib.stream_ptr(stream)), "rgbm_v1_point_rows")
        self._last_v1 = (feat, ch, Pv, dep, homog, scratch)      # keep inputs and scratch alive until the stream has consumed them
        return fused, nocs4, rows, planes

    def fetch(self, B: int, name: str, max_elems: int) -> torch.Tensor:
        """Debug/test access to a named intermediate of the last forward (fp32, flat)."""
        if self._last_split:
            raise _lib.RgbmError("fetch: the last forward ran as two half batches (split_streams); run it with split_streams=False for taps")
        if self._last_graph:
            raise _lib.RgbmError("fetch: the last forward replayed a captured graph (its intermediates live in the graph's own workspace); "
                                 "run it with graph=False for taps")
        buf = torch.empty(max_elems, dtype=torch.float32, device=self.device)
        n = C.c_size_t()
        ws_ptr, _ = self._workspace(B)
        _lib.check(self.lib.rgbm_adapose_fetch(self._h, B, C.c_void_p(ws_ptr), name.encode(), _lib.ptr(buf), max_elems,
                                               C.byref(n), _lib.stream_ptr()), "rgbm_adapose_fetch")
        return buf[: n.value]


def postprocess(view1_nocs, view1_depth, view1_r, view1_choose, K_crop, E1, img_size: int = 224, stream=None):
    """Device post-processing: returns (bbox_world [B,8,3] f64, ts [B,4] f64, valid [B] i32) CUDA tensors.

    Mirrors the tail of `AdaPoseEstimator_v5.predict` (`interface_v5.py:318-321,354-374`)."""
    lib = _lib.load()
    dev = view1_nocs.device
    B, P = view1_depth.shape
    nocs = view1_nocs.to(torch.float32).contiguous()
    depth = view1_depth.to(torch.float32).contiguous()
    r = view1_r.to(torch.float32).contiguous()
    ch = torch.as_tensor(view1_choose).to(device=dev, dtype=torch.int32).contiguous()
    K = torch.as_tensor(K_crop).to(device=dev, dtype=torch.float64).contiguous()
    E = torch.as_tensor(E1).to(device=dev, dtype=torch.float64).contiguous()
    bbox = torch.empty(B, 8, 3, dtype=torch.float64, device=dev)
    ts = torch.empty(B, 4, dtype=torch.float64, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    # small batches: the exact-median search is sliced over several workgroups per pose (needs device scratch; bit-identical)
    nb = C.c_size_t()
    _lib.check(lib.rgbm_adapose_postprocess_scratch_bytes(B, C.byref(nb)), "rgbm_adapose_postprocess_scratch_bytes")
    scratch = torch.empty(nb.value // 8, dtype=torch.int64, device=dev) if nb.value else None
    if scratch is not None and stream is not None:
        scratch.record_stream(stream)      # allocated on the current stream, used (and dropped on return) on `stream`: the caching allocator must not reuse it early
    _lib.check(lib.rgbm_adapose_postprocess_ws(B, P, img_size, _lib.ptr(nocs), _lib.ptr(depth), _lib.ptr(r), _lib.ptr(ch),
                                               _lib.ptr(K), _lib.ptr(E), _lib.ptr(bbox), _lib.ptr(ts), _lib.ptr(valid),
                                               _lib.ptr(scratch), nb.value, _lib.stream_ptr(stream)), "rgbm_adapose_postprocess_ws")
    return bbox, ts, valid


def view_fusion(net, x1, x2, stream=None):
    """`AdaPoseNet.view_fusion`: the attention stack of a baseline `net` on rows x1 / x2 [B, P, 32] -> (y1, y2) float32 CUDA."""
    return net.view_fusion(x1, x2, stream=stream)


def depth_head(net, x, stream=None):
    """`AdaPoseNet.depth_head`: depth_head of a baseline `net` on rows x [..., 32] -> [...] float32 CUDA."""
    return net.depth_head(x, stream=stream)


def view_fusion_ref(state_dict, x1, x2, prefix: str = "view_fusion.", stats: dict | None = None):
    """float64 numpy twin of `view_fusion` (tests, documentation): lib/fusion.py:11-82 as network_baseline.py:631 calls it (no mask, no
    position embedding, no dropout).  state_dict: the baseline net's (numpy or torch values, optional `module.` prefix); rows x1 / x2
    [B, P, 32] -> (y1, y2) [B, P, 32] float64.  Both attentions of a block read the block's inputs.  stats (optional dict) receives
    `rowmax` (mean largest probability per row), `score_absmax`, `score_min` and `score_max` per attention, fusion1 then fusion2 of every block."""
    sd = {}
    for k, v in state_dict.items():
        k = k[7:] if k.startswith("module.") else k
        if k.startswith(prefix):
            sd[k[len(prefix):]] = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    B, P, _ = x1.shape

    def attend(xq, xkv, p):
        lin = lambda i, x: x @ sd[f"{p}.linears.{i}.weight"].T + sd[f"{p}.linears.{i}.bias"]
        q, k, v = (lin(i, x).reshape(B, P, 4, 8).transpose(0, 2, 1, 3) for i, x in ((0, xq), (1, xkv), (2, xkv)))
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(8.0)                     # [B, 4, P, P]
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        pr = e / e.sum(axis=-1, keepdims=True)
        if stats is not None:
            stats.setdefault("rowmax", []).append(float(pr.max(axis=-1).mean()))
            stats.setdefault("score_absmax", []).append(float(np.abs(s).max()))
            stats.setdefault("score_min", []).append(float(s.min()))
            stats.setdefault("score_max", []).append(float(s.max()))
        return lin(3, (pr @ v).transpose(0, 2, 1, 3).reshape(B, P, 32))
    for blk in range(4):
        y1 = attend(x1, x2, f"blocks.{blk}.fusion1") + x1
        y2 = attend(x2, x1, f"blocks.{blk}.fusion2") + x2
        x1, x2 = y1, y2
    return x1, x2


def nocs_map(net, feat, stream=None):
    """`AdaPoseNet.nocs_map`: the NOCS branch of `net` at every row of feat [V, HW, 32] -> [V, HW, 3] float32 CUDA."""
    return net.nocs_map(feat, stream=stream)


def postprocess_regressed(view1_nocs, view1_r, view1_t, view1_s, E1, stream=None):
    """Device tail of `AdaPoseEstimator_v4.predict` for `direct_regression: True` (`interface_v4.py:322-325, 358-378`): translation
    view1_t and scale ||view1_s|| from the network's own heads, no pair median.  Returns (bbox_world [B,8,3] f64, ts [B,4] f64 =
    t xyz, scale, valid [B] i32) CUDA tensors; one launch for any B >= 1 and 1 <= P <= 1024, no scratch."""
    lib = _lib.load()
    dev = view1_nocs.device
    B, P = view1_nocs.shape[:2]
    f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    nocs, r, t, s = f32(view1_nocs), f32(view1_r), f32(view1_t), f32(view1_s)
    assert nocs.shape == (B, P, 3) and r.shape == (B, 3, 3) and t.shape == (B, 3) and s.shape == (B, 3), (nocs.shape, r.shape, t.shape, s.shape)
    E = torch.as_tensor(E1).to(device=dev, dtype=torch.float64).contiguous()
    assert E.shape == (B, 4, 4), E.shape
    bbox = torch.empty(B, 8, 3, dtype=torch.float64, device=dev)
    ts = torch.empty(B, 4, dtype=torch.float64, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.rgbm_adapose_postprocess_regressed(B, P, _lib.ptr(nocs), _lib.ptr(r), _lib.ptr(t), _lib.ptr(s), _lib.ptr(E), _lib.ptr(bbox),
                                                      _lib.ptr(ts), _lib.ptr(valid), _lib.stream_ptr(stream)), "rgbm_adapose_postprocess_regressed")
    return bbox, ts, valid


def postprocess_ransac(view1_nocs, view1_depth, view1_choose, K_crop, E1, img_size: int = 224, seed: int = 0, stream=None):
    """Device tail of `predict` for `direct_regression: False`, `use_depth: True` (`interface_v5.py:322-339, 348-374`,
    `lib/align.py:10-104`): returns (bbox_world [B,8,3] f64, srt [B,13] f64 = scale, R, t, valid [B] i32) CUDA tensors."""
    lib = _lib.load()
    dev = view1_nocs.device
    B, P = view1_depth.shape
    nocs = view1_nocs.to(torch.float32).contiguous()
    depth = view1_depth.to(torch.float32).contiguous()
    ch = torch.as_tensor(view1_choose).to(device=dev, dtype=torch.int32).contiguous()
    K = torch.as_tensor(K_crop).to(device=dev, dtype=torch.float64).contiguous()
    E = torch.as_tensor(E1).to(device=dev, dtype=torch.float64).contiguous()
    bbox = torch.empty(B, 8, 3, dtype=torch.float64, device=dev)
    srt = torch.empty(B, 13, dtype=torch.float64, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.rgbm_adapose_postprocess_ransac(B, P, img_size, int(seed) & 0xFFFFFFFF, _lib.ptr(nocs), _lib.ptr(depth),
                                                   _lib.ptr(ch), _lib.ptr(K), _lib.ptr(E), _lib.ptr(bbox), _lib.ptr(srt),
                                                   _lib.ptr(valid), _lib.stream_ptr(stream)), "rgbm_adapose_postprocess_ransac")
    return bbox, srt, valid


def postprocess_pnp(view1_nocs, view1_pts2d, view2_nocs, view2_pts2d, K, E1, E2, seed: int = 0, stream=None):
    """Device tail of `predict` for `direct_regression: False`, `use_depth: False` (`interface_v5.py:340-346`, `lib/utils.py:121-195`,
    `lib/align.py:104-115`): returns (bbox_world [B,8,3] f64, srt [B,13] f64 = scale, R, t, info [B,4] i32 = matches / RANSAC ok /
    inliers / hypotheses examined, valid [B] i32) CUDA tensors.  pts2d: pixels of the chosen points in the ORIGINAL frame."""
    lib = _lib.load()
    dev = view1_nocs.device
    B, P = view1_nocs.shape[:2]
    f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    f64 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
    n1, p1, n2, p2 = f32(view1_nocs), f32(view1_pts2d), f32(view2_nocs), f32(view2_pts2d)
    Kd, E1d, E2d = f64(K), f64(E1), f64(E2)
    bbox = torch.empty(B, 8, 3, dtype=torch.float64, device=dev)
    srt = torch.empty(B, 13, dtype=torch.float64, device=dev)
    info = torch.empty(B, 4, dtype=torch.int32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.rgbm_adapose_postprocess_pnp(B, P, int(seed) & 0xFFFFFFFF, _lib.ptr(n1), _lib.ptr(p1), _lib.ptr(n2), _lib.ptr(p2),
                                                _lib.ptr(Kd), _lib.ptr(E1d), _lib.ptr(E2d), _lib.ptr(bbox), _lib.ptr(srt), _lib.ptr(info),
                                                _lib.ptr(valid), _lib.stream_ptr(stream)), "rgbm_adapose_postprocess_pnp")
    return bbox, srt, info, valid


def postprocess_pnp_scaled(view1_nocs, view1_pts2d, view1_s, K, E1, seed: int = 0, stream=None):
    """Device tail of `AdaPoseEstimator_realworld.predict` (`interface_realworld.py:295-320`): scale = ||view1_s|| in float32, then
    `postprocess_pnp`'s steps from EPnP-RANSAC on with view 1 alone.  Returns (bbox_world [B,8,3] f64, srt [B,13] f64 = scale, R, t,
    info [B,4] i32 = P / RANSAC ok / inliers / hypotheses examined, valid [B] i32) CUDA tensors.  view1_s [B,3] float32 (the network's
    regressed size); pts2d: pixels of the chosen points in the ORIGINAL frame; K the original intrinsics.  5 <= P <= 1024."""
    lib = _lib.load()
    dev = view1_nocs.device
    B, P = view1_nocs.shape[:2]
    f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    f64 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
    n1, p1, s1 = f32(view1_nocs), f32(view1_pts2d), f32(view1_s)
    Kd, E1d = f64(K), f64(E1)
    bbox = torch.empty(B, 8, 3, dtype=torch.float64, device=dev)
    srt = torch.empty(B, 13, dtype=torch.float64, device=dev)
    info = torch.empty(B, 4, dtype=torch.int32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.rgbm_adapose_postprocess_pnp_scaled(B, P, int(seed) & 0xFFFFFFFF, _lib.ptr(n1), _lib.ptr(p1), _lib.ptr(s1), _lib.ptr(Kd),
                                                       _lib.ptr(E1d), _lib.ptr(bbox), _lib.ptr(srt), _lib.ptr(info), _lib.ptr(valid),
                                                       _lib.stream_ptr(stream)), "rgbm_adapose_postprocess_pnp_scaled")
    return bbox, srt, info, valid


def pts2d_to_coor(pts2d, W: int, H: int, stream=None):
    """pts2d [..., 2] float32 CUDA (pixels in a W x H frame) -> (x / W, y / H) float32, the real-world network's coordinate inputs
    (`interface_realworld.py:264-269`); true float32 divisions, equal to numpy's bit for bit."""
    lib = _lib.load()
    t = torch.as_tensor(pts2d).to(dtype=torch.float32).contiguous()
    out = torch.empty_like(t)
    _lib.check(lib.rgbm_pts2d_to_coor(_lib.ptr(t), _lib.ptr(out), t.numel() // 2, int(W), int(H), _lib.stream_ptr(stream)), "rgbm_pts2d_to_coor")
    return out


def prepare_inputs(rgb, mask, K, img_size: int = 224, n_pts: int = 1024, seed: int = 0, want_pts2d: bool = False, stream=None,
                   frame_map=None, frame0: int = 0, normalize: bool = True, want_mask: bool = False, sample: str = "resized"):
    """Batched device-side `AdaPoseEstimator_v5.prepare_model_input` (`interface_v5.py:58-170`).

    rgb [N,H,W,3] float32 in [0,1], mask [N,H,W] (0/1), K [N,3,3]: torch CUDA tensors (or anything torch.as_tensor accepts).
    A torch.uint8 rgb (a camera's bytes) is read as it is (`rgbm_prepare_inputs_u8`): byte b is the pixel fl32(b / 255), so every
    output equals bit for bit what the float32 frames b / 255 give, without a float32 copy of the frames.
    With `frame_map` [N] int32, rgb / mask are a pool [M,H,W,..] (e.g. a view queue) and frame f reads entry frame_map[f]
    (negative: no view -> valid 0) — no gather of the selected frames is needed; K stays [N,3,3].
    `normalize=False` (`rgbm_prepare_inputs_opt`): img is the resized crop itself, without the ImageNet mean / std step — the plain
    `ToTensor` transform of `AdaPoseEstimator_v4` for every task but "pots" (`interface_v4.py:52-58`); every other output is unchanged.
    `want_mask=True` adds `mask` [N,S,S] uint8: the nearest-neighbour resize of the frame mask's crop window that `choose` is drawn from.
    `sample="native"` (`rgbm_prepare_inputs_native`; `AdaPoseEstimator_v2.prepare_model_input`, `interface_v2.py:74-98`): the points are drawn
    from the frame mask at native resolution inside the crop window (candidate i = row * crop_w + col, the same seeded subset rule on i)
    and mapped into the crop afterwards: pts2d are whole pixels of the frame, choose = floor(row * ratio) * S + floor(col * ratio) with
    ratio = S / crop_w, which repeats when the window is larger than the crop.  img, Kcrop and window are unchanged.
    Returns dict(img [N,3,S,S] f32, choose [N,P] i32, Kcrop [N,3,3] f64, window [N,4] i32, valid [N] i32[, pts2d][, mask])."""
    lib = _lib.load()
    dev = rgb.device if isinstance(rgb, torch.Tensor) and rgb.is_cuda else torch.device("cuda", torch.cuda.current_device())
    rgb = torch.as_tensor(rgb)
    u8 = rgb.dtype == torch.uint8
    rgb = rgb.to(device=dev, dtype=torch.uint8 if u8 else torch.float32).contiguous()
    mask = torch.as_tensor(mask).to(device=dev)
    if mask.dtype != torch.uint8:                       # the kernels test for non-zero, so a uint8 mask is used as it is
        mask = (mask != 0).to(torch.uint8)
    mask = mask.contiguous()
    K = torch.as_tensor(K).to(device=dev, dtype=torch.float64).contiguous()
    _, H, W, _ = rgb.shape
    N = K.shape[0]
    if frame_map is None:
        assert rgb.shape[0] == N and mask.shape[0] == N
    else:
        frame_map = torch.as_tensor(frame_map).to(device=dev, dtype=torch.int32).contiguous()
        assert frame_map.shape == (N,) and mask.shape[0] == rgb.shape[0]
    S, P = int(img_size), int(n_pts)
    img = torch.empty(N, 3, S, S, dtype=torch.float32, device=dev)
    choose = torch.empty(N, P, dtype=torch.int32, device=dev)
    pts2d = torch.empty(N, P, 2, dtype=torch.float32, device=dev) if want_pts2d else None
    Kcrop = torch.empty(N, 3, 3, dtype=torch.float64, device=dev)
    window = torch.empty(N, 4, dtype=torch.int32, device=dev)
    valid = torch.empty(N, dtype=torch.int32, device=dev)
    scratch = torch.empty(N * S * S, dtype=torch.uint8, device=dev)
    tail = (N, H, W, S, P, int(seed) & 0xFFFFFFFF, _lib.ptr(img), _lib.ptr(choose), _lib.ptr(pts2d), _lib.ptr(Kcrop), _lib.ptr(window),
            _lib.ptr(valid), _lib.ptr(scratch), _lib.stream_ptr(stream))
    if sample not in ("resized", "native"):
        raise ValueError(f"prepare_inputs: sample must be 'resized' or 'native', got {sample!r}")
    if sample == "native":
        _lib.check(lib.rgbm_prepare_inputs_native(_lib.ptr(rgb), int(u8), int(bool(normalize)), _lib.ptr(mask), _lib.ptr(K), _lib.ptr(frame_map),
                                                  int(frame0), *tail), "rgbm_prepare_inputs_native")
    elif not normalize:
        _lib.check(lib.rgbm_prepare_inputs_opt(_lib.ptr(rgb), int(u8), 0, _lib.ptr(mask), _lib.ptr(K), _lib.ptr(frame_map), int(frame0), *tail),
                   "rgbm_prepare_inputs_opt")
    elif u8:
        _lib.check(lib.rgbm_prepare_inputs_u8(_lib.ptr(rgb), _lib.ptr(mask), _lib.ptr(K), _lib.ptr(frame_map), int(frame0), *tail),
                   "rgbm_prepare_inputs_u8")
    elif frame0:        # a piece of a larger batch: frame f hashes as frame frame0 + f of the whole batch would
        _lib.check(lib.rgbm_prepare_inputs_ex(_lib.ptr(rgb), _lib.ptr(mask), _lib.ptr(K), _lib.ptr(frame_map), int(frame0), *tail),
                   "rgbm_prepare_inputs_ex")
    elif frame_map is None:
        _lib.check(lib.rgbm_prepare_inputs(_lib.ptr(rgb), _lib.ptr(mask), _lib.ptr(K), *tail), "rgbm_prepare_inputs")
    else:
        _lib.check(lib.rgbm_prepare_inputs_indexed(_lib.ptr(rgb), _lib.ptr(mask), _lib.ptr(K), _lib.ptr(frame_map), *tail),
                   "rgbm_prepare_inputs_indexed")
    out = {"img": img, "choose": choose, "Kcrop": Kcrop, "window": window, "valid": valid}
    if want_pts2d:
        out["pts2d"] = pts2d
    if want_mask:
        out["mask"] = scratch.view(N, S, S)
    return out


def prepare_inputs_windows(pix, mask_pix, offset, window, valid_in, K, H: int, W: int, img_size: int = 224, n_pts: int = 1024, seed: int = 0,
                           want_pts2d: bool = False, stream=None, frame0: int = 0, normalize: bool = True, want_mask: bool = False):
    """`prepare_inputs` from crop windows the host has cut out of the frames and packed (`rgbm_prepare_inputs_windows`, cfg hip_upload:
    "windows"; upload.mask_windows / pack_windows): pix flat float32 or uint8 (3 elements per pixel), mask_pix flat uint8, offset [N]
    int64 (pixel offset of frame f's window in both), window [N,4] int32, valid_in [N] int32 (0: empty mask) — CUDA tensors; K [N,3,3];
    H, W: the size of the frames the windows were cut from.  Returns the dict of `prepare_inputs`, bit for bit what it returns for the
    whole frames (its "window" is the tensor handed in; `want_mask` as there)."""
    lib = _lib.load()
    dev = pix.device
    if pix.dtype not in (torch.uint8, torch.float32) or mask_pix.dtype != torch.uint8:
        raise TypeError(f"prepare_inputs_windows: pix float32 or uint8 and mask_pix uint8, got {pix.dtype} / {mask_pix.dtype}")
    N = int(window.shape[0])
    K = torch.as_tensor(K).to(device=dev, dtype=torch.float64).contiguous()
    offset = offset.to(device=dev, dtype=torch.int64).contiguous()
    window = window.to(device=dev, dtype=torch.int32).contiguous()
    valid_in = valid_in.to(device=dev, dtype=torch.int32).contiguous()
    assert K.shape[0] == N and offset.shape == (N,) and window.shape == (N, 4) and valid_in.shape == (N,)
    assert pix.is_contiguous() and mask_pix.is_contiguous() and pix.numel() == 3 * mask_pix.numel()
    S, P = int(img_size), int(n_pts)
    img = torch.empty(N, 3, S, S, dtype=torch.float32, device=dev)
    choose = torch.empty(N, P, dtype=torch.int32, device=dev)
    pts2d = torch.empty(N, P, 2, dtype=torch.float32, device=dev) if want_pts2d else None
    Kcrop = torch.empty(N, 3, 3, dtype=torch.float64, device=dev)
    valid = torch.empty(N, dtype=torch.int32, device=dev)
    scratch = torch.empty(N * S * S, dtype=torch.uint8, device=dev)
    _lib.check(lib.rgbm_prepare_inputs_windows(_lib.ptr(pix), int(pix.dtype == torch.uint8), int(bool(normalize)), _lib.ptr(mask_pix), _lib.ptr(offset),
                                               _lib.ptr(window), _lib.ptr(valid_in), _lib.ptr(K), int(frame0), N, int(H), int(W), S, P,
                                               int(seed) & 0xFFFFFFFF, _lib.ptr(img), _lib.ptr(choose), _lib.ptr(pts2d), _lib.ptr(Kcrop), _lib.ptr(valid),
                                               _lib.ptr(scratch), _lib.stream_ptr(stream)), "rgbm_prepare_inputs_windows")
    out = {"img": img, "choose": choose, "Kcrop": Kcrop, "window": window, "valid": valid}
    if want_pts2d:
        out["pts2d"] = pts2d
    if want_mask:
        out["mask"] = scratch.view(N, S, S)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Host mirror of the device's dependency cone (csrc/prob_sparse.hip::cone_of), for reporting and capacity planning: which part of
# the plane-sweep volume the network needs for a given set of chosen pixels (option "sparse_dec"; network_v5.py:260-291, 449-455).
def needed_c0_interval(y: int, S: int = 224):
    """Index interval [lo, hi] of c0 (full resolution, one axis) that the probabilities of a pixel at coordinate y depend on."""
    def clamp(a, b, n):
        return max(a, 0), min(b, n - 1)
    tr = lambda o, n: clamp(o[0] >> 1, (o[1] + 1) >> 1, n)      # noqa: E731  ConvTranspose3d k3 s2 p1 op1
    s1 = lambda o, n: clamp(o[0] - 1, o[1] + 1, n)              # noqa: E731  Conv3d k3 p1
    s2 = lambda o, n: clamp(2 * o[0] - 1, 2 * o[1] + 1, n)      # noqa: E731  Conv3d k3 p1 stride 2
    u = lambda p, q: (min(p[0], q[0]), max(p[1], q[1]))         # noqa: E731
    u11 = clamp(y - 1, y + 1, S)
    u9 = tr(u11, S // 2)
    u7 = tr(u9, S // 4)
    c5 = s1(tr(u7, S // 8), S // 8)
    c4 = u(s2(c5, S // 4), u7)
    c2 = u(s2(s1(c4, S // 4), S // 2), u9)
    return u(s2(s1(c2, S // 2), S), u11)


def sweep_tiles_needed_fraction(choose, S: int = 224, th: int = 12, tw: int = 16) -> float:
    """Fraction of the depth-sweeping conv0's th x tw-pixel tiles inside the dependency cones of the chosen pixels; choose [V, P]."""
    ch = np.asarray(choose.cpu() if isinstance(choose, torch.Tensor) else choose).reshape(-1, np.asarray(choose.shape)[-1])
    lo = np.array([needed_c0_interval(v, S)[0] for v in range(S)])
    hi = np.array([needed_c0_interval(v, S)[1] for v in range(S)])
    nth, ntw = -(-S // th), -(-S // tw)
    total = 0
    for row in ch:
        y, x = row // S, row % S
        m = np.zeros((nth, ntw), bool)
        for ra, rb, ca, cb in set(zip(lo[y] // th, hi[y] // th, lo[x] // tw, hi[x] // tw)):
            m[ra:rb + 1, ca:cb + 1] = True
        total += int(m.sum())
    return total / (len(ch) * nth * ntw)

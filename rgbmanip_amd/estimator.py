"""`pose_estimator=adapose_*` plugin: AdaPoseEstimator_v5 and AdaPoseEstimator_v4 on the HIP network.

Mirrors `/root/reference/models/pose_estimator/AdaPose/interface_v5.py:37-374` and the base class
`models/pose_estimator/base_estimator.py:5-20`: `AdaPoseEstimator_v5(env, cfg, logger)`,
`estimate(K, rgb1, mask1, E1, rgb2, mask2, E2) -> ndarray [N,8,3]`, `predict(...)`, `prepare_model_input(...)`,
never raises for bad samples (empty mask / non-finite result -> `default_bbox`, the +10 cube).

Differences that are the point of this build: `estimate` prepares all N samples, runs ONE batched network call and ONE
batched post-processing launch on the device instead of N serial B=1 calls with a host round trip each
(interface_v5.py:218-225, 259-286, 318-321), and it skips `draw_result` (a discarded debug drawing, :364).
The crop/resize/sampling step runs on the host in numpy by default (the reference's arithmetic incl. its global-RNG
subset) or, with cfg["hip_prepare"] == "device", batched on the GPU (`rgbm_prepare_inputs`; the 1024-subset
is then a seeded hash, cfg["hip_prepare_seed"]); `estimate_device` takes device-resident frames and never leaves the GPU.

`AdaPoseEstimator_v4` (`interface_v4.py:37-378`, `pose_estimator.name: adapose_v4`) is the same network (lib/network_v4.py is
lib/network_v5.py bar one blank line) behind an interface that differs in two places, the two hooks of the class below: the crops are
ImageNet-normalised only for task "pots" (`interface_v4.py:52-58`), and the `direct_regression: True` tail takes translation and scale
from the network's own heads (`interface_v4.py:322-325`, `rgbm_adapose_postprocess_regressed`) instead of the pair median.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from functools import partial

import numpy as np
import torch

from . import _lib, host_prepare
from . import samples as samples_mod
from . import verify as verify_mod
from .adapose import (AdaPoseNet, postprocess, postprocess_pnp, postprocess_pnp_scaled, postprocess_ransac, postprocess_regressed, prepare_inputs,
                      prepare_inputs_windows, pts2d_to_coor)
from .cloud import (DEFAULT_BBOX, cloud_gather, cloud_gather_views, cloud_pack, cloud_pack_views, cloud_similarity, depth_consistency, depth_fusion,
                    depth_to_points)
from .feature_cache import CachedViews, ContentFeatureCache, SlotFeatureCache
from .host_prepare import _resize_linear, _resize_nearest, get_bbox      # noqa: F401  (part of this module's surface)
from .upload import (ChunkPipeline, WindowRing, _nonzero_into, _split, frames_payload_bytes, frames_to_device, host_array,      # noqa: F401
                     masks_to_device)

_DEPTH_PLANES = np.arange(0.1, 0.1 * (24 - 0.5) + 0.1, 0.1, dtype=np.float32)      # the 24 sweep depths (interface_v5.py:259-262)


def _put(out, a, b, res):
    """Rows a .. b - 1 of a pipelined call's result: the boxes, or every tensor of `estimate_depth`'s dict."""
    if isinstance(out, dict):
        for k, v in out.items():
            v[a:b] = res[k]
    else:
        out[a:b] = res


@dataclass(frozen=True)
class ResultPlan:
    """What a two-view call returns, on its way through upload, chunk pipeline, network and tails (`want=`): the boxes of `estimate` (the
    default instance), the dict of `estimate_depth` (`maps`), that dict extended by `estimate_cloud` (`maps` and `cloud`, under the
    thresholds and the capacity below), and with a `fit_seed` the fit of `estimate_cloud_pose` on top."""
    maps: bool = False                 # the dense maps: the network runs densely and on the plain path (the content cache is bypassed)
    cloud: bool = False                # ... checked against each other and packed (with maps only)
    px_max: float = 1.0
    rel_max: float = 0.01
    conf_min: float = 0.0
    masked: bool = True
    cap: int | None = 0                # rows of the packed cloud
    fit_seed: int | None = None        # seed of the similarity fit; None: no fit

    @property
    def fit(self) -> bool:
        """`cloud_similarity` runs on the cloud's NOCS rows, after the chunks."""
        return self.fit_seed is not None

    @property
    def prepare_kw(self) -> dict:
        """Extra keywords of `_prepare` / `_prepare_windows`."""
        return {"want_mask": True} if self.cloud else {}

    @property
    def network_kw(self) -> dict:
        """Extra keywords of the network call."""
        if not self.maps:
            return {}
        return {"dense_depth": True, "dense_nocs": True} if self.fit else {"dense_depth": True}


@dataclass(frozen=True)
class ViewsPlan(ResultPlan):
    """The plan of `estimate_cloud_views`: every frame's maps, fused where `n_min` sources agree; cap None: V S S."""
    maps: bool = True
    n_min: int = 1


BOXES = ResultPlan()


def _to_host(out):
    return {k: v.cpu().numpy() for k, v in out.items()} if isinstance(out, dict) else out.cpu().numpy()


class BasePoseEstimator:
    def __init__(self, env, cfg: dict, logger):
        self.env = env
        self.cfg = cfg
        self.logger = logger

    def append_picture(self, pic, pose):
        pass

    def estimate(self):
        pass


def dropout_cfg(cfg) -> tuple:
    """(hip_norm_mode, hip_dropout, hip_dropout_seed) of an estimator cfg.  hip_as_shipped: true is the reference as shipped
    (interface_v5.py:39-56 never calls .eval(), rl_pose.py predicts one pose per call): per-sample BatchNorm3d statistics and
    PSPNet's Dropout2d(p = 0.15) — shorthand for hip_norm_mode: per_sample + hip_dropout: 0.15; keys given explicitly win."""
    shipped = bool(cfg.get("hip_as_shipped", False))
    norm_mode = cfg.get("hip_norm_mode", "per_sample" if shipped else "eval")
    p = float(cfg.get("hip_dropout", 0.15 if shipped else 0.0))
    if not (p == 0.0 or 0.0 < p < 1.0):
        raise ValueError(f"hip_dropout must be 0 (off) or lie in (0, 1), got {p}")
    return norm_mode, p, int(cfg.get("hip_dropout_seed", 0))


def _check_shared_net(net, view2_heads, drop_p, drop_seed, want):
    """A shared network keeps ITS settings (changing them on the shared handle would drop every captured graph and change the other
    users' outputs): refuse a cfg that needs others.  `want`: the cfg's hip_options.  Returns the net's view2_heads."""
    # the combination that would feed never-written view-2 outputs to the PnP tail
    net_v2 = bool(net.options.get("view2_heads", 1))
    if view2_heads and not net_v2:
        raise ValueError("AdaPoseEstimator_v5: this cfg needs the view-2 heads (hip_view2_heads, or the PnP tail of "
                         "direct_regression=False / use_depth=False), but the shared net was built with view2_heads=0")
    # ... and Dropout2d: the shared handle draws one mask sequence (resetting it here would restart the other users' sequence)
    if float(np.float32(net.dropout)) != float(np.float32(drop_p)) or (drop_p > 0 and net.dropout_seed != drop_seed):
        raise ValueError(f"AdaPoseEstimator_v5: this cfg asks for dropout p={drop_p} seed={drop_seed} (hip_dropout / hip_as_shipped), "
                         f"but the shared net runs p={net.dropout} seed={net.dropout_seed}")
    # ... and the same for hip_options: a key this cfg names must already hold on the shared net (round-5 advice: silently
    # ignoring e.g. {"sweep_f16": 0} would run the f16 feature map the user opted out of)
    differ = {k: (v, net.options.get(k)) for k, v in want.items() if net.options.get(k) != v}
    if differ:
        raise ValueError("AdaPoseEstimator_v5: cfg.hip_options is not applied to a shared net; build the AdaPoseNet with "
                         f"options={want} (requested vs the net's: {differ})")
    return net_v2


class AdaPoseEstimator_v5(BasePoseEstimator):
    _CHUNK_BYTES = 64 << 20           # staging rows of _upload_frames
    _frame = 0                        # hash-subset mode of prepare_model_input: index of the sample being prepared

    def __init__(self, env, cfg, logger, state_dict=None, dtype=None, device=0, net=None):
        """`net`: an already built `AdaPoseNet` to share (weights + workspace) instead of building one from `state_dict`."""
        super().__init__(env, cfg, logger)
        # hip_upload (estimate() with host arrays and hip_prepare: device): "frames" (default) stages and uploads every pixel of every
        # frame; "windows" derives each frame's crop window from its mask on the host and uploads only that part of the frame and of the
        # mask (upload.WindowRing, rgbm_prepare_inputs_windows) — the same boxes bit for bit, 22 % of the bytes on the crop test frames
        self.upload_mode = cfg.get("hip_upload", "frames")
        if self.upload_mode not in ("frames", "windows"):
            raise ValueError(f'AdaPoseEstimator_v5: hip_upload is "frames" or "windows", got {self.upload_mode!r}')
        if self.upload_mode == "windows" and cfg.get("hip_prepare", "device") != "device":
            raise ValueError('AdaPoseEstimator_v5: hip_upload: "windows" packs the crop windows for the device-side preparation; it needs '
                             f'hip_prepare: "device", got {cfg.get("hip_prepare")!r}')
        self.upload_bytes_last_call = 0       # payload the last estimate() handed to the copy engine: frames and masks, or their windows
        self.upload_table_bytes_last_call = 0         # ... and the offset / window / valid tables on top of it (hip_upload: "windows")
        if net is not None:
            state_dict = {}
        elif state_dict is None:
            if cfg.get("load", False):
                state_dict = torch.load(cfg["checkpoint_path"], map_location="cpu")      # DataParallel keys ("module.")
            else:
                state_dict = self._synthetic_state_dict()
                if logger is not None:
                    logger.warning(f"{type(self).__name__}: cfg.load is False -> synthetic (seeded) weights")
        self.dtype = dtype or cfg.get("hip_dtype", "bf16x3")      # the fastest mode inside north_star's 1e-4 (fp32: 4x slower, bf16: 2.4x faster at 1e-2)
        # hip_graph (default off: measured, small batches are bound by their kernels, not by the ~100 launches): batches of at most
        # hip_graph_max_batch poses replay a captured hipGraph.
        # hip_view2_heads (default: only where the box tail reads view-2 outputs, i.e. the PnP branch): the reference network returns
        # ten outputs and `predict` builds the box from view1_nocs / view1_depth / view1_r alone (interface_v5.py:318-374; v4's regressed
        # tail: view1_nocs / view1_r / view1_t / view1_s, interface_v4.py:322-325), so the cost volume, point heads and pose regression of
        # the view-2 crops are skipped — the backbone still runs on both views, and all five view-1 outputs are computed in either mode
        self.view2_heads = bool(cfg.get("hip_view2_heads", self._pnp_branch()))
        # hip_dropout / hip_dropout_seed / hip_as_shipped (dropout_cfg): PSPNet's Dropout2d, seeded, fresh masks on every forward
        norm_mode, drop_p, drop_seed = dropout_cfg(cfg)
        # hip_feature_cache (default off): `estimate_device_indexed(..., fresh=...)` keeps every pool frame's PSPNet feature map in a
        # record pool and runs the PSPNet only on the frames named fresh (DESIGN.md "Feature cache").  Dropout2d draws its masks per pose
        # and per forward, so a kept map would change what the as-shipped estimator computes: the combination is refused.
        # "content" is True plus the same for `estimate` / `estimate_device`, whose frames arrive as fresh arrays: every prepared crop is
        # fingerprinted on the device (rgbm_crop_fingerprint), a host table (feature_keys.py) maps key -> record of a pool of
        # hip_feature_cache_records records (0: twice the poses of the largest call so far), and the PSPNet runs on the crops not met before
        mode = cfg.get("hip_feature_cache", False)
        if isinstance(mode, str) and mode != "content":
            raise ValueError(f'AdaPoseEstimator_v5: hip_feature_cache is False, True or "content", got {mode!r}')
        self.feature_cache = bool(mode)
        self.feature_content = mode == "content"
        if self.feature_cache and drop_p > 0:
            raise ValueError("AdaPoseEstimator_v5: hip_feature_cache keeps feature maps across forwards, Dropout2d (hip_dropout / "
                             f"hip_as_shipped: p={drop_p}) draws fresh masks on every forward; turn one of them off")
        records = int(cfg.get("hip_feature_cache_records", 0))
        if records < 0:
            raise ValueError(f"hip_feature_cache_records must be 0 (twice the poses of the largest call) or a record count, got {records}")
        # hip_options: any rgbm_adapose_set_option key (include/rgbm.h), e.g. {"sweep_f16": 0} for a bf16 checkpoint whose 32-channel
        # feature map can exceed the f16 range (the plane sweep of bf16 nets reads it as f16 since round 5)
        options = {str(k): int(v) for k, v in dict(cfg.get("hip_options", {}) or {}).items()}
        if net is not None:
            self.view2_heads = _check_shared_net(net, self.view2_heads, drop_p, drop_seed, options)      # report what the net computes
        self.estimator = net if net is not None else self._build_net(state_dict, device, norm_mode, drop_p, drop_seed,
                                                                     {**options, "view2_heads": int(self.view2_heads)})
        self._plain_views = 0                 # views the PSPNet has run on in uncached forwards
        self.frames_u8_native = 0             # frames the device paths have cropped straight from 8-bit pixels (rgbm_prepare_inputs_u8)
        self._slots = SlotFeatureCache(self.estimator, self._normalize)                 # estimate_device_indexed(..., fresh=...)
        self._content = ContentFeatureCache(self.estimator, records)     # estimate / estimate_device with "content"
        self._ring = self._pipe = None        # staging of _upload_frames / of the chunk pipeline, built by the first call that needs them
        self._wring = None                    # one-slot WindowRing of an unchunked hip_upload: "windows" call
        self._dev_consts = None               # (DEFAULT_BBOX, _DEPTH_PLANES) on the device
        self._pnp_warned = False
        self.rng = np.random          # the reference shuffles with the global numpy RNG (interface_v5.py:129)
        # "device" (default since round 5): frames are uploaded once and cropped / resized / sub-sampled on the GPU (rgbm_prepare_inputs);
        # a mask with more than 1024 pixels keeps the 1024 smallest hash keys (hip_prepare_seed) instead of the pixels np.random.shuffle
        # would pick (interface_v5.py:126-130) — same distribution, another stream.  "host": the reference's per-frame numpy path on the
        # global numpy RNG (one host core: 46 ms per pose), for RNG-stream parity with the reference.
        self.prepare_mode = cfg.get("hip_prepare", "device")
        self.prepare_seed = int(cfg.get("hip_prepare_seed", 0))

    @property
    def feature_views_computed(self):
        """Views the PSPNet has run on through this estimator's device paths."""
        return self._plain_views + self._slots.views_computed + self._content.views_computed

    @property
    def feature_cache_bypassed(self):
        return self._content.bypassed

    # ------------------------------------------------------------------ the network construction (what the baseline interface overrides)
    def _synthetic_state_dict(self):
        from . import synth
        return synth.adapose_state_dict(seed=0)

    def _build_net(self, state_dict, device, norm_mode, drop_p, drop_seed, options):
        return AdaPoseNet(state_dict, dtype=self.dtype, device=device, norm_mode=norm_mode, dropout=drop_p, dropout_seed=drop_seed,
                          graph=bool(self.cfg.get("hip_graph", False)), graph_max_batch=int(self.cfg.get("hip_graph_max_batch", 32)),
                          options=options)

    # ------------------------------------------------------------------ the two places where the v4 interface differs
    @property
    def _normalize(self) -> bool:
        """ImageNet mean / std on the crops (interface_v5.py:52-54: always)."""
        return True

    def _regressed_tail(self, pred, choose, Kcrop, E1):
        """The `direct_regression: True` box: scale = exact median over the point pairs, translation from it (interface_v5.py:318-321)."""
        return postprocess(pred["view1_nocs"], pred["view1_depth"], pred["view1_r"], choose, Kcrop, E1, img_size=self.cfg["img_size"])[0]

    # ------------------------------------------------------------------ interface_v5.py:58-170
    def prepare_model_input(self, rgb, mask, intrinsic, resize_size):
        return host_prepare.prepare_model_input(rgb, mask, intrinsic, resize_size, self.rng, self._frame, normalize=self._normalize)

    # ------------------------------------------------------------------ interface_v5.py:213-227
    def estimate(self, camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch,
                 view2_mask_batch, view2_extrinsic_batch):
        S = self.cfg["img_size"]
        n = len(rgb1_batch)
        if self.prepare_mode == "device":
            return self._estimate_host_frames(camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch,
                                              view2_mask_batch, view2_extrinsic_batch, want=BOXES)
        out = np.repeat(DEFAULT_BBOX[None], n, axis=0)
        rows, img1, img2, ch1, ch2, P1, P2, K1, E1 = [], [], [], [], [], [], [], [], []
        pt1, pt2, E2, K0 = [], [], [], []                    # the PnP branch also needs the pixels, the second extrinsic and the original K
        # a user-set ("hash", s) means "hash subset"; its seeds are the device path's: prepare_seed for view 1, + 1 for view 2
        rng1, rng2 = (("hash", self.prepare_seed), ("hash", self.prepare_seed + 1)) if isinstance(self.rng, tuple) else (self.rng, self.rng)
        for i in range(n):
            a = host_prepare.prepare_model_input(rgb1_batch[i], view1_mask_batch[i], camera_intrinsic_batch[i], S, rng1, i, normalize=self._normalize)
            b = host_prepare.prepare_model_input(rgb2_batch[i], view2_mask_batch[i], camera_intrinsic_batch[i], S, rng2, i, normalize=self._normalize)
            if a[0] is None or b[0] is None:
                continue
            p1, p2 = np.eye(4), np.eye(4)
            p1[:3, :] = a[3] @ np.asarray(view1_extrinsic_batch[i])[:3, :]
            p2[:3, :] = b[3] @ np.asarray(view2_extrinsic_batch[i])[:3, :]
            rows.append(i)
            img1.append(a[0].float()); img2.append(b[0].float())
            ch1.append(a[1]); ch2.append(b[1])
            P1.append(p1.astype(np.float32)); P2.append(p2.astype(np.float32))
            K1.append(a[3]); E1.append(np.asarray(view1_extrinsic_batch[i], dtype=np.float64))
            pt1.append(a[2]); pt2.append(b[2]); E2.append(np.asarray(view2_extrinsic_batch[i], dtype=np.float64))
            K0.append(np.asarray(camera_intrinsic_batch[i], dtype=np.float64))
        if not rows:
            return out
        depths = np.tile(_DEPTH_PLANES[None], (len(rows), 1))
        ch1 = np.stack(ch1)
        pred = self.estimator(torch.stack(img1), ch1, torch.stack(img2), np.stack(ch2), np.stack(P1), np.stack(P2), depths)
        bbox = self._bbox_tail(pred, ch1, np.stack(K1), np.stack(E1), pts2d=(np.stack(pt1), np.stack(pt2)), E2=np.stack(E2), K=np.stack(K0))
        out[np.asarray(rows)] = bbox.cpu().numpy()
        return out

    # ------------------------------------------------------------------ host frames -> HBM (upload.py)
    def _estimate_host_frames(self, K, rgb1, mask1, E1, rgb2, mask2, E2, want: ResultPlan):
        """`estimate` with `hip_prepare: device`: one `estimate_device` call, or for more than `hip_upload_chunk` host poses the
        chunk pipeline (upload.ChunkPipeline), whose per-chunk work is defined here.  `want`: the boxes, or the dict of `estimate_depth`
        / `estimate_cloud` instead (plain path: no content cache)."""
        n = len(rgb1)
        chunk = int(self.cfg.get("hip_upload_chunk", 32))
        cuda = [isinstance(x, torch.Tensor) and x.is_cuda for x in (rgb1, rgb2, mask1, mask2)]
        if self.upload_mode == "windows" and not any(cuda):
            return self._estimate_host_windows(K, rgb1, mask1, E1, rgb2, mask2, E2, n, chunk, want=want)
        self.upload_bytes_last_call, self.upload_table_bytes_last_call = frames_payload_bytes(rgb1, rgb2, mask1, mask2), 0
        # boxes: the public entry point, so that what a subclass or a test puts in its place is what runs
        on_device = partial(self._estimate_device, want=want) if want.maps else self.estimate_device
        if cuda[0] or cuda[1] or n <= chunk or chunk <= 0:
            return _to_host(self._cloud_fit(on_device(np.asarray(K), self._upload_frames(rgb1), self._upload_masks(mask1), np.asarray(E1),
                                                      self._upload_frames(rgb2), self._upload_masks(mask2), np.asarray(E2)), want=want))
        dev = self.estimator.device
        srcs = [host_array(x) for x in (rgb1, rgb2, mask1, mask2)]
        pipe = self._pipe = ChunkPipeline.matching(self._pipe, chunk, srcs, dev)
        Kd = torch.as_tensor(np.asarray(K)).to(dev)
        E1d, E2d = torch.as_tensor(np.asarray(E1)).to(dev), torch.as_tensor(np.asarray(E2)).to(dev)
        out = self._alloc_out(n=n, dev=dev, want=want)
        if self.feature_content and not want.maps:
            self._content.reserve(n)
            S, wp = self.cfg["img_size"], self._pnp_branch()

            def prepare(a, b, d):
                pa = self._prepare(self._upload_frames(d[0]), d[2], Kd[a:b], S, 1024, self.prepare_seed, want_pts2d=wp, frame0=a)
                pb = self._prepare(self._upload_frames(d[1]), d[3], Kd[a:b], S, 1024, self.prepare_seed + 1, want_pts2d=wp, frame0=a)
                return a, b, self._content.keys(pa, pb)

            def network(p):
                a, b, keys = p
                out[a:b] = self._estimate_keyed(keys, E1d[a:b], E2d[a:b], Kd[a:b])
            pipe.run_keyed(srcs, n, prepare, network)
        else:
            def network(a, b, d):
                _put(out, a, b, on_device(Kd[a:b], self._upload_frames(d[0]), d[2], E1d[a:b], self._upload_frames(d[1]), d[3], E2d[a:b], frame0=a))
            pipe.run(srcs, n, network)
        res = _to_host(self._cloud_fit(out, want=want))
        pipe.trace.report(self.upload_bytes_last_call)
        return res

    def _estimate_host_windows(self, K, rgb1, mask1, E1, rgb2, mask2, E2, n, chunk, want: ResultPlan):
        """`_estimate_host_frames` with hip_upload: "windows": the host derives every frame's crop window from its mask, packs that part of
        the frame and of the mask into pinned staging and uploads the packed buffers (upload.WindowRing); `rgbm_prepare_inputs_windows`
        writes img / choose / pts2d / Kcrop / valid from them and everything behind is the code of the whole-frame path.  At most
        `hip_upload_chunk` poses (or chunk 0): the whole call is packed at once; more: the chunk pipeline with a window ring."""
        dev = self.estimator.device
        srcs = [host_array(x) for x in (rgb1, rgb2, mask1, mask2)]
        Kd = torch.as_tensor(np.asarray(K)).to(dev)
        E1d, E2d = torch.as_tensor(np.asarray(E1)).to(dev), torch.as_tensor(np.asarray(E2)).to(dev)
        S, wp = self.cfg["img_size"], self._pnp_branch()
        cached = self.feature_content and not want.maps

        def prep(a, b, d):
            return [self._prepare_windows(d, v, Kd[a:b], S, 1024, self.prepare_seed + v, want_pts2d=wp, frame0=a, **want.prepare_kw) for v in (0, 1)]
        if n <= chunk or chunk <= 0:
            ring = self._wring = WindowRing.matching(self._wring, n, srcs, dev, slots=1, grow=True)
            ring.payload_bytes = ring.table_bytes = 0
            ring.wait(0)
            ring.stage(0, srcs, 0, n)
            pa, pb = prep(0, n, ring.copy(0, n))
            if cached:
                self._content.reserve(n)
                out = self._estimate_keyed(self._content.keys(pa, pb), E1d, E2d, Kd)
            else:
                out = self._estimate_prepared(pa, pb, E1d, E2d, Kd, want=want)
            res = _to_host(self._cloud_fit(out, want=want))
            self.upload_bytes_last_call, self.upload_table_bytes_last_call = ring.payload_bytes, ring.table_bytes
            return res
        pipe = self._pipe = ChunkPipeline.matching(self._pipe, chunk, srcs, dev, windows=True)
        ring = pipe.ring
        ring.payload_bytes = ring.table_bytes = 0
        out = self._alloc_out(n=n, dev=dev, want=want)
        if cached:
            self._content.reserve(n)

            def prepare(a, b, d):
                return a, b, self._content.keys(*prep(a, b, d))

            def network(p):
                a, b, keys = p
                out[a:b] = self._estimate_keyed(keys, E1d[a:b], E2d[a:b], Kd[a:b])
            pipe.run_keyed(srcs, n, prepare, network)
        else:
            def network(a, b, d):
                pa, pb = prep(a, b, d)
                _put(out, a, b, self._estimate_prepared(pa, pb, E1d[a:b], E2d[a:b], Kd[a:b], want=want))
            pipe.run(srcs, n, network)
        res = _to_host(self._cloud_fit(out, want=want))
        self.upload_bytes_last_call, self.upload_table_bytes_last_call = ring.payload_bytes, ring.table_bytes
        pipe.trace.report(self.upload_bytes_last_call)
        return res

    def _prepare_windows(self, d, v, K, *args, **kw):
        """`prepare_inputs_windows` on view v of a `PackedViews`, counting the frames cropped straight from bytes like `_prepare`."""
        out = prepare_inputs_windows(d.pix[v], d.mask[v], d.offset[v], d.window[v], d.valid[v], K, d.H, d.W, *args, normalize=self._normalize, **kw)
        if d.pix[v].dtype == torch.uint8:
            self.frames_u8_native += int(out["img"].shape[0])
        return out

    def _upload_frames(self, frames):
        out, self._ring = frames_to_device(frames, self.estimator.device, self._ring, self._CHUNK_BYTES, keep_u8=True)
        return out

    def _prepare(self, rgb, *args, **kw):
        """`prepare_inputs`, counting the frames it crops straight from bytes (uint8 frames stay uint8 all the way into the kernel)."""
        out = prepare_inputs(rgb, *args, normalize=self._normalize, **kw)
        if getattr(rgb, "dtype", None) == torch.uint8:
            self.frames_u8_native += int(out["img"].shape[0])
        return out

    def _upload_masks(self, masks):
        return masks_to_device(masks, self.estimator.device)

    # ------------------------------------------------------------------ the same pipeline without leaving the device
    def estimate_device(self, K, rgb1, mask1, E1, rgb2, mask2, E2, frame0: int = 0):
        """`estimate` for frames that already live on the GPU (or get uploaded once): K [N,3,3], rgb [N,H,W,3] float32 in [0,1] or
        uint8 (byte b = the pixel fl32(b / 255); read as bytes, same boxes bit for bit), mask [N,H,W], E [N,4,4] world->camera.
        Returns a CUDA tensor [N,8,3] float64; samples the reference would skip
        (empty mask) or reject (non-finite box) hold `default_bbox`."""
        return self._estimate_device(K, rgb1, mask1, E1, rgb2, mask2, E2, frame0=frame0, want=BOXES)

    def _estimate_device(self, K, rgb1, mask1, E1, rgb2, mask2, E2, frame0: int = 0, *, want: ResultPlan):
        S, dev = self.cfg["img_size"], self.estimator.device
        Kd = torch.as_tensor(K).to(dev)
        kw = dict(want_pts2d=self._pnp_branch(), frame0=frame0, **want.prepare_kw)
        a = self._prepare(torch.as_tensor(rgb1).to(dev), torch.as_tensor(mask1).to(dev), Kd, S, 1024, self.prepare_seed, **kw)
        b = self._prepare(torch.as_tensor(rgb2).to(dev), torch.as_tensor(mask2).to(dev), Kd, S, 1024, self.prepare_seed + 1, **kw)
        if self.feature_content and not want.maps:      # one host synchronisation per call: the keys must be on the host before the network can be enqueued
            self._content.reserve(int(Kd.shape[0]))
            return self._estimate_keyed(self._content.keys(a, b), E1, E2, Kd)
        return self._estimate_prepared(a, b, E1, E2, Kd, want=want)

    # ------------------------------------------------------------------ dense depth of the view-1 crops (DESIGN.md "Dense depth maps")
    def estimate_depth(self, camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch,
                       view2_mask_batch, view2_extrinsic_batch):
        """`estimate` (same arguments, frame dtypes, hip_upload modes and chunk pipeline) returning what the cost volume holds for the
        view-1 crop of every sample, as a dict of numpy arrays: `bbox` [n,8,3] f64 (the box `estimate` builds from the dense-tail
        outputs), `depth` / `conf` [n,S,S] f32 (expected depth and largest plane probability at every pixel of the crop), `points`
        [n,S,S,3] f32 (the depth map back-projected into the world frame), `window` [n,4] i32 (rmin, rmax, cmin, cmax: where the crop
        lies in the frame), `Kcrop` [n,3,3] f64 (the crop's intrinsics), `valid` [n] i32.  A sample with an empty mask has valid 0, NaN
        maps and the +10 cube.  The network runs densely and on the plain path: cfg hip_feature_cache is bypassed for this call
        (counted in `feature_cache_bypassed`), hip_graph is ignored."""
        if self.prepare_mode != "device":
            raise ValueError(f'estimate_depth crops on the device: it needs hip_prepare: "device", got {self.prepare_mode!r}')
        return self._estimate_host_frames(camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch,
                                          view2_mask_batch, view2_extrinsic_batch, want=ResultPlan(maps=True))

    def estimate_depth_device(self, K, rgb1, mask1, E1, rgb2, mask2, E2, frame0: int = 0):
        """`estimate_depth` for frames that live on the GPU (the arguments of `estimate_device`): the same dict, as CUDA tensors."""
        return self._estimate_device(K, rgb1, mask1, E1, rgb2, mask2, E2, frame0=frame0, want=ResultPlan(maps=True))

    # ------------------------------------------------------------------ consistent two-view point cloud
    def _cloud_options(self, px_max, rel_max, conf_min, masked, max_points, **fit) -> ResultPlan:
        if self.prepare_mode != "device":
            raise ValueError(f'estimate_cloud crops on the device: it needs hip_prepare: "device", got {self.prepare_mode!r}')
        if not self.view2_heads:
            raise ValueError("estimate_cloud checks the view-1 depth map against the view-2 map: it needs a net that runs the view-2 heads "
                             "(cfg hip_view2_heads: True; the default for the regression tail is False)")
        cap = 2 * self.cfg["img_size"] ** 2 if max_points is None else int(max_points)
        if cap < 0:
            raise ValueError(f"estimate_cloud: max_points >= 0, got {max_points}")
        seed = int(self.cfg.get("hip_ransac_seed", 0) if fit["fit_seed"] is None else fit["fit_seed"]) if fit else None      # estimate_cloud_pose
        return ResultPlan(True, True, float(px_max), float(rel_max), float(conf_min), bool(masked), cap, seed)

    def estimate_cloud(self, camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch, view2_mask_batch,
                       view2_extrinsic_batch, *, px_max=1.0, rel_max=0.01, conf_min=0.0, masked=True, max_points=None):
        """`estimate_depth` (same arguments, frame types, upload modes and chunk pipeline) followed by the two-view geometric consistency
        check and the packed point cloud of the pixels that pass it, as a dict of numpy arrays.  Everything `estimate_depth` returns,
        unchanged, plus `depth2` / `conf2` [n,S,S] f32, `window2` [n,4] i32, `Kcrop2` [n,3,3] f64 (the same for the view-2 crop), `mask1` /
        `mask2` [n,S,S] u8 (the crop-resolution masks `choose` is drawn from), `fused1` / `reproj1` / `rel1` [n,S,S] f32 and `keep1`
        [n,S,S] u8 (`depth_consistency` of view 1 against view 2; `...2`: view 2 against view 1), `cloud` [n,cap,3] f32, `cloud_index`
        [n,cap] i32 and `count` [n,2] i32 (`cloud_pack`: view 1's kept pixels in row-major order, then view 2's; cap = max_points, default
        2 S S).  A pixel is kept when it comes back within `px_max` pixels at a depth within `rel_max`, with confidence >= `conf_min`
        and, with `masked`, inside its crop mask.  A sample with valid 0 has keep 0, count [0, 0] and NaN maps and cloud rows.  Needs the
        view-2 maps, i.e. cfg hip_view2_heads: True, and hip_prepare: "device"; the feature cache is bypassed as in `estimate_depth`."""
        return self._estimate_host_frames(camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch, view2_mask_batch,
                                          view2_extrinsic_batch, want=self._cloud_options(px_max, rel_max, conf_min, masked, max_points))

    def estimate_cloud_device(self, K, rgb1, mask1, E1, rgb2, mask2, E2, frame0: int = 0, *, px_max=1.0, rel_max=0.01, conf_min=0.0,
                              masked=True, max_points=None):
        """`estimate_cloud` for frames that live on the GPU (the arguments of `estimate_device`): the same dict, as CUDA tensors."""
        return self._estimate_device(K, rgb1, mask1, E1, rgb2, mask2, E2, frame0=frame0,
                                     want=self._cloud_options(px_max, rel_max, conf_min, masked, max_points))

    # ------------------------------------------------------------------ a box fitted to the two-view cloud
    def estimate_cloud_pose(self, camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch, view2_mask_batch,
                            view2_extrinsic_batch, *, px_max=1.0, rel_max=0.01, conf_min=0.0, masked=True, max_points=None, fit_seed=None,
                            verify=False, inflate=0.0):
        """`estimate_cloud` (same arguments, keywords, frame types, upload modes, chunk pipeline and errors) plus the object-space
        coordinate of every cloud row and a second, independent box per pose fitted to them.  Everything `estimate_cloud` returns,
        unchanged, plus `nocs1` / `nocs2` [n,S,S,3] f32 (the network's NOCS branch at every pixel of the two crops; read at `choose` they
        are the point NOCS), `cloud_nocs` [n,cap,3] f32 (the maps at `cloud_index`), and the similarity RANSAC of the reference's
        `direct_regression: False` tail between `cloud_nocs` and `cloud` (`cloud_similarity`, seed `fit_seed`, default cfg
        hip_ransac_seed; pose b of the call draws stream b, whatever the chunking): `bbox_cloud` [n,8,3] f64 (world frame), `srt_cloud`
        [n,13] f64 (scale, R, t), `fit_info` [n,4] i32 (rows used, kept hypothesis or -1, its inliers, hypotheses examined) and
        `valid_cloud` [n] i32.  A sample with valid 0, fewer than 5 rows or no consensus has valid_cloud 0 and the +10 cube; a sample with
        valid 0 has NaN NOCS maps.  `verify`: the two boxes are checked against the frame masks and the cloud (`verify.cloud_pose_verify`
        with `inflate`; hypothesis 0 is `bbox`, 1 is `bbox_cloud`) and the dict gains `mask_iou` [n,2,2] f64 (box, view), `mask_score`
        [n,2] f64, `cloud_share` [n,2] f64 and `best` [n] i64 (-1: neither box is usable); the uint8 masks are uploaded once more for it."""
        r = self._estimate_host_frames(camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch, view2_mask_batch,
                                       view2_extrinsic_batch, want=self._cloud_options(px_max, rel_max, conf_min, masked, max_points, fit_seed=fit_seed))
        if verify:
            r = self._cloud_pose_verified(r, camera_intrinsic_batch, view1_extrinsic_batch, self._upload_masks(view1_mask_batch),
                                          view2_extrinsic_batch, self._upload_masks(view2_mask_batch), inflate)
        return r

    def estimate_cloud_pose_device(self, K, rgb1, mask1, E1, rgb2, mask2, E2, frame0: int = 0, *, px_max=1.0, rel_max=0.01, conf_min=0.0,
                                   masked=True, max_points=None, fit_seed=None, verify=False, inflate=0.0):
        """`estimate_cloud_pose` for frames that live on the GPU (the arguments of `estimate_device`): the same dict, as CUDA tensors."""
        opts = self._cloud_options(px_max, rel_max, conf_min, masked, max_points, fit_seed=fit_seed)
        dev = self.estimator.device
        mask1, mask2 = torch.as_tensor(mask1).to(dev), torch.as_tensor(mask2).to(dev)
        r = self._cloud_fit(self._estimate_device(K, rgb1, mask1, E1, rgb2, mask2, E2, frame0=frame0, want=opts), want=opts)
        return self._cloud_pose_verified(r, K, E1, mask1, E2, mask2, inflate) if verify else r

    @staticmethod
    def _cloud_pose_verified(r, K, E1, mask1, E2, mask2, inflate):
        """r plus the keys of `verify=True`: numpy for a dict of numpy arrays, CUDA tensors for one of CUDA tensors."""
        v = verify_mod.cloud_pose_verify(r, np.asarray(K) if not isinstance(K, torch.Tensor) else K, E1, mask1, E2, mask2, inflate=inflate)
        r = dict(r)
        r.update(mask_iou=v["iou"], mask_score=v["score"], cloud_share=v["share"], best=v["best"])
        return r

    def _cloud_fit(self, out, want: ResultPlan):
        """The fit of `estimate_cloud_pose` over all poses of a call at once (so that pose b draws sample stream b however the call was
        chunked); every other result passes through untouched."""
        if not want.fit:
            return out
        bbox, srt, info, valid = cloud_similarity(out["cloud_nocs"], out["cloud"], out["count"], seed=want.fit_seed)
        out = dict(out)
        out.update(bbox_cloud=bbox, srt_cloud=srt, fit_info=info, valid_cloud=valid)
        return out

    def _cloud_tail(self, r, pred, a, b, E1d, E2d, ok, o: ResultPlan):
        """The dict of `estimate_depth` (r, left as it is) extended by the view-2 maps, the two checks and the packed cloud."""
        n = E1d.shape[0]
        nan = torch.full((), float("nan"), dtype=torch.float32, device=E1d.device)
        d2 = torch.where(ok.view(n, 1, 1), pred["view2_depth_map"], nan)
        c2 = torch.where(ok.view(n, 1, 1), pred["view2_depth_conf"], nan)
        th = dict(px_max=o.px_max, rel_max=o.rel_max, conf_min=o.conf_min)
        m1, m2 = (a["mask"], b["mask"]) if o.masked else (None, None)
        v1 = depth_consistency(r["depth"], a["Kcrop"], E1d, d2, b["Kcrop"], E2d, conf_a=r["conf"], mask_a=m1, **th)
        v2 = depth_consistency(d2, b["Kcrop"], E2d, r["depth"], a["Kcrop"], E1d, conf_a=c2, mask_a=m2, **th)
        cloud, index, count = cloud_pack(v1["fused"], v1["keep"], a["Kcrop"], E1d, v2["fused"], v2["keep"], b["Kcrop"], E2d, max_points=o.cap)
        r.update(depth2=d2, conf2=c2, window2=b["window"], Kcrop2=b["Kcrop"], mask1=a["mask"], mask2=b["mask"], cloud=cloud,
                 cloud_index=index, count=count)
        for v, res in ((1, v1), (2, v2)):
            for k in ("fused", "keep", "reproj", "rel"):
                r[f"{k}{v}"] = res[k]
        if o.fit:
            n1 = torch.where(ok.view(n, 1, 1, 1), pred["view1_nocs_map"], nan)
            n2 = torch.where(ok.view(n, 1, 1, 1), pred["view2_nocs_map"], nan)
            r.update(nocs1=n1, nocs2=n2, cloud_nocs=cloud_gather(n1, n2, index))
        return r

    # ------------------------------------------------------------------ V views of a pose: fused maps, one cloud, one box
    _VIEWS_CHUNK = 64                 # network poses per dense forward of estimate_cloud_views

    def _views_options(self, n_min, px_max, rel_max, conf_min, masked, max_points, fit, fit_seed):
        if self.prepare_mode != "device":
            raise ValueError(f'estimate_cloud_views crops on the device: it needs hip_prepare: "device", got {self.prepare_mode!r}')
        if self.upload_mode == "windows":
            raise ValueError('estimate_cloud_views uploads whole frames: cfg hip_upload: "windows" is not implemented for it (use "frames")')
        if max_points is not None and int(max_points) < 0:
            raise ValueError(f"estimate_cloud_views: max_points >= 0, got {max_points}")
        seed = int(self.cfg.get("hip_ransac_seed", 0) if fit_seed is None else fit_seed) if fit else None
        return ViewsPlan(px_max=float(px_max), rel_max=float(rel_max), conf_min=float(conf_min), masked=bool(masked),
                         cap=None if max_points is None else int(max_points), fit_seed=seed, n_min=int(n_min))

    def estimate_cloud_views(self, K, frames, masks, E, *, n_min=1, px_max=1.0, rel_max=0.01, conf_min=0.0, masked=True, max_points=None,
                             fit=False, fit_seed=None):
        """One cloud (and, with `fit`, one box) per pose from V >= 2 frames of it: K [n,3,3], frames [n,V,H,W,3] (float64 / float32 in
        [0,1] or uint8), masks [n,V,H,W], E [n,V,4,4] world -> camera.  Every frame is uploaded and cropped once; frame k then runs
        through the dense forward of `estimate_depth` as view 1 of a network pose whose view 2 is its neighbour p(k) (p(k) = k + 1, and
        p(V - 1) = V - 2); the n V view-1 maps go through `depth_fusion` (every pixel checked against the other V - 1 views, kept when at
        least `n_min` agree within `px_max` pixels / `rel_max` relative depth, with confidence >= `conf_min` and, with `masked`, inside
        its crop mask) and `cloud_pack_views`.  Returns a dict of numpy arrays: `depth` / `conf` / `fused` [n,V,S,S] f32, `mask` / `keep`
        / `nviews` [n,V,S,S] u8, `agree` [n,V,S,S] int16 (bit b: view b agrees), `window` [n,V,4] i32, `Kcrop` [n,V,3,3] f64, `valid`
        [n,V] i32, `cloud` [n,cap,3] f32, `cloud_index` [n,cap] i32 (view * S * S + pixel), `count` [n,V] i32; cap = max_points, default
        V S S.  With `fit`: `nocs` [n,V,S,S,3] f32, `cloud_nocs` [n,cap,3] f32 and `bbox_cloud` / `srt_cloud` / `fit_info` / `valid_cloud`
        of `cloud_similarity` (seed `fit_seed`, default cfg hip_ransac_seed) on the cloud with its counts folded to [total, 0].  A frame
        whose own mask or whose neighbour's mask is empty has valid 0, NaN maps and keep 0, and agrees with nobody as a source.  Needs
        hip_prepare: "device" and whole-frame upload (hip_upload: "windows" is refused); the view-2 heads are not needed; the feature
        cache is bypassed and counted as in `estimate_depth`."""
        o = self._views_options(n_min, px_max, rel_max, conf_min, masked, max_points, fit, fit_seed)
        cuda = isinstance(frames, torch.Tensor) and frames.is_cuda
        fr = frames if cuda else host_array(frames)
        mk = masks if isinstance(masks, torch.Tensor) and masks.is_cuda else host_array(masks)
        if fr.ndim != 5 or mk.ndim != 4:
            raise ValueError(f"estimate_cloud_views: frames [n,V,H,W,3] and masks [n,V,H,W], got {tuple(fr.shape)} and {tuple(mk.shape)}")
        n, V = int(fr.shape[0]), int(fr.shape[1])
        flat_f, flat_m = fr.reshape((n * V,) + tuple(fr.shape[2:])), mk.reshape((n * V,) + tuple(mk.shape[2:]))
        self.upload_bytes_last_call, self.upload_table_bytes_last_call = frames_payload_bytes(flat_f, flat_f[:0], flat_m, flat_m[:0]), 0      # one stack of each
        fd, md = self._upload_frames(flat_f), self._upload_masks(flat_m)
        return _to_host(self._estimate_views(np.asarray(K), fd.view((n, V) + tuple(fd.shape[1:])), md.view((n, V) + tuple(md.shape[1:])),
                                             np.asarray(E), o))

    def estimate_cloud_views_device(self, K, frames, masks, E, *, n_min=1, px_max=1.0, rel_max=0.01, conf_min=0.0, masked=True,
                                    max_points=None, fit=False, fit_seed=None):
        """`estimate_cloud_views` for frames that live on the GPU (float32 or uint8 [n,V,H,W,3]): the same dict, as CUDA tensors."""
        return self._estimate_views(K, frames, masks, E, self._views_options(n_min, px_max, rel_max, conf_min, masked, max_points, fit, fit_seed))

    def _estimate_views(self, K, frames, masks, E, o):
        dev, S = self.estimator.device, self.cfg["img_size"]
        frames, masks = torch.as_tensor(frames).to(dev), torch.as_tensor(masks).to(dev)
        if frames.dim() != 5 or masks.dim() != 4 or masks.shape[:2] != frames.shape[:2]:
            raise ValueError(f"estimate_cloud_views: frames [n,V,H,W,3] and masks [n,V,H,W], got {tuple(frames.shape)} and {tuple(masks.shape)}")
        n, V = int(frames.shape[0]), int(frames.shape[1])
        if not 2 <= V <= 16 or not 1 <= o.n_min <= V - 1:
            raise ValueError(f"estimate_cloud_views: 2 <= V <= 16 and 1 <= n_min <= V - 1, got V = {V}, n_min = {o.n_min}")
        Kd = torch.as_tensor(K).to(device=dev, dtype=torch.float64)
        Ed = torch.as_tensor(E).to(device=dev, dtype=torch.float64)
        if tuple(Kd.shape) != (n, 3, 3) or tuple(Ed.shape) != (n, V, 4, 4):
            raise ValueError(f"estimate_cloud_views: K [n,3,3] and E [n,V,4,4], got {tuple(Kd.shape)} and {tuple(Ed.shape)}")
        N = n * V
        E1 = Ed.reshape(N, 4, 4)
        # every frame is cropped once, as a view 1 (its choose subset is drawn with the view-1 seed, also where it serves as a view 2)
        a = self._prepare(frames.reshape((N,) + tuple(frames.shape[2:])), masks.reshape((N,) + tuple(masks.shape[2:])),
                          Kd.repeat_interleave(V, dim=0), S, 1024, self.prepare_seed, want_mask=True)
        nb = torch.arange(N, device=dev).view(n, V)
        nb = torch.cat([nb[:, 1:], nb[:, V - 2:V - 1]], dim=1).reshape(N)      # p(k) = k + 1, p(V - 1) = V - 2
        b = {k: a[k].index_select(0, nb) for k in ("img", "choose", "Kcrop", "valid")}
        E2 = E1.index_select(0, nb)
        depth = torch.empty(N, S, S, dtype=torch.float32, device=dev)
        conf = torch.empty_like(depth)
        nocs = torch.empty(N, S, S, 3, dtype=torch.float32, device=dev) if o.fit else None
        for lo in range(0, N, self._VIEWS_CHUNK):
            hi = min(lo + self._VIEWS_CHUNK, N)
            rows = lambda d: {k: d[k][lo:hi] for k in ("img", "choose", "Kcrop")}      # noqa: E731
            pred = self._forward(rows(a), rows(b), E1[lo:hi], E2[lo:hi], o)
            depth[lo:hi], conf[lo:hi] = pred["view1_depth_map"], pred["view1_depth_conf"]
            if o.fit:
                nocs[lo:hi] = pred["view1_nocs_map"]
        ok = (a["valid"] != 0) & (b["valid"] != 0)
        nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        depth = torch.where(ok.view(N, 1, 1), depth, nan).view(n, V, S, S)
        conf = torch.where(ok.view(N, 1, 1), conf, nan).view(n, V, S, S)
        Kc, mask = a["Kcrop"].view(n, V, 3, 3), a["mask"].view(n, V, S, S)
        f = depth_fusion(depth, Kc, Ed, conf=conf, mask=mask if o.masked else None, px_max=o.px_max, rel_max=o.rel_max,
                         conf_min=o.conf_min, n_min=o.n_min)
        cloud, index, count = cloud_pack_views(f["fused"], f["keep"], Kc, Ed, max_points=o.cap)
        r = {"depth": depth, "conf": conf, "fused": f["fused"], "mask": mask, "keep": f["keep"], "nviews": f["nviews"], "agree": f["agree"],
             "window": a["window"].view(n, V, 4), "Kcrop": Kc, "valid": ok.to(torch.int32).view(n, V), "cloud": cloud, "cloud_index": index,
             "count": count}
        if o.fit:
            nocs = torch.where(ok.view(N, 1, 1, 1), nocs, nan).view(n, V, S, S, 3)
            cn = cloud_gather_views(nocs, index)
            folded = torch.stack([count.sum(dim=1, dtype=torch.int32), torch.zeros(n, dtype=torch.int32, device=dev)], dim=1)
            bbox, srt, info, valid = cloud_similarity(cn, cloud, folded, seed=o.fit_seed)
            r.update(nocs=nocs, cloud_nocs=cn, bbox_cloud=bbox, srt_cloud=srt, fit_info=info, valid_cloud=valid)
        return r

    def _alloc_out(self, n, dev, want: ResultPlan):
        """What the chunks of a pipelined call are written into: the boxes, the tensors of `estimate_depth`, or those of `estimate_cloud`."""
        f32, i32, f64, u8 = torch.float32, torch.int32, torch.float64, torch.uint8
        new = lambda dt, *shape: torch.empty(n, *shape, dtype=dt, device=dev)      # noqa: E731
        if not want.maps:
            return new(f64, 8, 3)
        S, cap = self.cfg["img_size"], want.cap
        out = {"bbox": new(f64, 8, 3), "depth": new(f32, S, S), "conf": new(f32, S, S), "points": new(f32, S, S, 3), "window": new(i32, 4),
               "Kcrop": new(f64, 3, 3), "valid": new(i32)}
        if want.cloud:
            out.update(depth2=new(f32, S, S), conf2=new(f32, S, S), window2=new(i32, 4), Kcrop2=new(f64, 3, 3), mask1=new(u8, S, S),
                       mask2=new(u8, S, S), cloud=new(f32, cap, 3), cloud_index=new(i32, cap), count=new(i32, 2))
            for v in (1, 2):
                out.update({f"fused{v}": new(f32, S, S), f"keep{v}": new(u8, S, S), f"reproj{v}": new(f32, S, S), f"rel{v}": new(f32, S, S)})
            if want.fit:
                out.update(nocs1=new(f32, S, S, 3), nocs2=new(f32, S, S, 3), cloud_nocs=new(f32, cap, 3))
        return out

    def estimate_device_indexed(self, K, rgb_pool, mask_pool, E1, E2, map1, map2, fresh=None):
        """`estimate_device` reading the two views of sample i from entries map1[i] / map2[i] of a frame pool
        (rgb_pool [M,H,W,3] float32 or uint8, mask_pool [M,H,W] uint8 — e.g. the controller's view queue) instead of from gathered
        batches; a negative entry means "no such view" (the reference hands an all-zero frame over, which is skipped).
        K [N,3,3] (both views use it, interface_v5.py:213-227), E1 / E2 [N,4,4].

        With cfg hip_feature_cache, `fresh` (a host sequence of pool entries; None = today's path) names the entries whose frames were
        written since their features were last computed: the PSPNet runs on exactly those len(fresh) views, their records are marked
        valid, and the network runs from the records of map1 / map2.  A pose that refers to an entry without a valid record gets
        `default_bbox`.  The caller owns the bookkeeping: an entry rewritten without being named keeps its old frame's map
        (`invalidate_features` forgets all of them)."""
        S = self.cfg["img_size"]
        wp = self._pnp_branch()
        cached = None
        if self.feature_cache and fresh is not None:
            cached = self._slots.update(rgb_pool, mask_pool, S, fresh, map1, map2, self.prepare_seed)
        a = self._prepare(rgb_pool, mask_pool, K, S, 1024, self.prepare_seed, frame_map=map1, want_pts2d=wp)
        b = self._prepare(rgb_pool, mask_pool, K, S, 1024, self.prepare_seed + 1, frame_map=map2, want_pts2d=wp)
        return self._estimate_prepared(a, b, E1, E2, K, cached=cached, want=BOXES)

    def invalidate_features(self):
        """Forget every cached feature map (the frame pool is about to be rewritten: `ControlInterface.reset_queue`)."""
        self._slots.invalidate()
        self._content.invalidate()

    def _estimate_keyed(self, pend, E1, E2, K):
        """The network for the views of `ContentFeatureCache.keys`, from the cache's records; a call with more distinct crops than
        records (finish: None) runs the plain path, bit for bit."""
        return self._estimate_prepared(pend.a, pend.b, E1, E2, K, cached=self._content.finish(pend), want=BOXES)

    def _pnp_branch(self):
        return not self.cfg.get("direct_regression", True) and not self.cfg.get("use_depth", True)

    def _consts(self, dev):
        """(DEFAULT_BBOX, _DEPTH_PLANES) on the device: a pageable host -> device copy per call would block the host until the stream has
        drained, i.e. serialise the chunk pipeline of _estimate_host_frames (measured: staging, copy and kernels ran back to back)."""
        if self._dev_consts is None or self._dev_consts[0].device != dev:
            self._dev_consts = (torch.from_numpy(DEFAULT_BBOX).to(dev), torch.from_numpy(_DEPTH_PLANES).to(dev))
        return self._dev_consts

    def _projection(self, Kc, E):
        """P = K' E[:3], padded to 4x4 (interface_v5.py:264-270), fp64 -> fp32."""
        n = int(E.shape[0])
        P = torch.empty(n, 4, 4, dtype=torch.float32, device=E.device)
        _lib.check(_lib.load().rgbm_projection(_lib.ptr(Kc.contiguous()), _lib.ptr(E.contiguous()), _lib.ptr(P), n, _lib.stream_ptr()), "rgbm_projection")
        return P

    def _forward(self, a, b, E1, E2, want: ResultPlan, cached: CachedViews | None = None):
        """The network on the prepared views a / b: from the cache's records, or from the crops as `want` says, which the two counters count."""
        n = int(E1.shape[0])
        P1, P2 = self._projection(a["Kcrop"], E1), self._projection(b["Kcrop"], E2)
        depths = self._consts(E1.device)[1][None].expand(n, 24).contiguous()
        if cached is not None:
            return self.estimator.forward_cached(cached.pool, cached.slot1, cached.slot2, a["choose"], b["choose"], P1, P2, depths)
        pred = self.estimator(a["img"], a["choose"], b["img"], b["choose"], P1, P2, depths, **want.network_kw, **self._network_inputs(a, b))
        self._plain_views += 2 * n
        if want.maps:
            self._content.bypassed += int(self.feature_cache)      # a call / chunk the cache was set for and did not serve
        return pred

    def _network_inputs(self, a, b) -> dict:
        """What the network reads of the prepared views beyond crops, chosen pixels and projections (the real-world interface: coordinates)."""
        return {}

    def _estimate_prepared(self, a, b, E1, E2, K=None, cached: CachedViews | None = None, *, want: ResultPlan):
        dev = self.estimator.device
        E1d = torch.as_tensor(E1).to(device=dev, dtype=torch.float64)
        E2d = torch.as_tensor(E2).to(device=dev, dtype=torch.float64)
        n = E1d.shape[0]
        assert cached is None or not want.maps
        pred = self._forward(a, b, E1d, E2d, want, cached)
        bbox = self._bbox_tail(pred, a["choose"], a["Kcrop"], E1d, pts2d=(a.get("pts2d"), b.get("pts2d")), E2=E2d, K=K)
        ok = (a["valid"] != 0) & (b["valid"] != 0)
        if cached is not None and cached.ok is not None:
            ok = ok & cached.ok
        box = torch.where(ok.view(n, 1, 1), bbox, self._consts(dev)[0].expand(n, 8, 3))
        if not want.maps:
            return box
        nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        depth = torch.where(ok.view(n, 1, 1), pred["view1_depth_map"], nan)
        conf = torch.where(ok.view(n, 1, 1), pred["view1_depth_conf"], nan)
        res = {"bbox": box, "depth": depth, "conf": conf, "points": depth_to_points(depth, a["Kcrop"], E1d),      # NaN depth -> NaN points
               "window": a["window"], "Kcrop": a["Kcrop"], "valid": ok.to(torch.int32)}
        return self._cloud_tail(res, pred, a, b, E1d, E2d, ok, want) if want.cloud else res

    def _bbox_tail(self, pred, choose, Kcrop, E1, pts2d=None, E2=None, K=None):
        """interface_v5.py:318-374: scale / translation from the regressed rotation (`direct_regression`, the shipped configs)
        or Umeyama-RANSAC between predicted NOCS and the back-projected predicted depth (`use_depth`), then the world box."""
        S = self.cfg["img_size"]
        if self.cfg.get("direct_regression", True):
            return self._regressed_tail(pred, choose, Kcrop, E1)
        if self.cfg.get("use_depth", True):
            return postprocess_ransac(pred["view1_nocs"], pred["view1_depth"], choose, Kcrop, E1, img_size=S,
                                      seed=int(self.cfg.get("hip_ransac_seed", 0)))[0]
        # use_depth False (interface_v5.py:340-346): NOCS matches of the two views -> scale -> EPnP-RANSAC + VVS on the ORIGINAL
        # intrinsics and the chosen points' pixels in the original frame
        if not self._pnp_warned:
            self._pnp_warned = True
            msg = ("AdaPoseEstimator_v5: direct_regression=False with use_depth=False runs csrc/pnp.hip, a restatement of OpenCV's "
                   "triangulatePoints / solvePnPRansac(EPNP) / solvePnPRefineVVS whose RANSAC subset stream and tie-breaks are NOT "
                   "pinned against cv2 (no OpenCV in the build image; DESIGN.md section 2): poses agree with ground truth, inlier sets "
                   "may differ from the reference's")
            warnings.warn(msg, RuntimeWarning, stacklevel=2)
            if self.logger is not None:
                self.logger.warning(msg)
        return postprocess_pnp(pred["view1_nocs"], pts2d[0], pred["view2_nocs"], pts2d[1], K, E1, E2,
                               seed=int(self.cfg.get("hip_ransac_seed", 0)))[0]

    def predict(self, camera_intrinsic, rgb1, view1_mask, view1_extrinsic, rgb2, view2_mask, view2_extrinsic):
        return self.estimate([camera_intrinsic], [rgb1], [view1_mask], [view1_extrinsic], [rgb2], [view2_mask],
                             [view2_extrinsic])[0]

    # ------------------------------------------------------------------ S Dropout2d samples per pose
    _SAMPLE_ROWS = 256                # network poses (samples x poses) per forward_samples call

    def _samples_check(self, samples, select=None) -> int:
        if select not in (None, "mask"):
            raise ValueError(f'estimate_samples: select must be None or "mask", got {select!r}')
        if self.feature_cache:
            raise ValueError("estimate_samples: cfg hip_feature_cache keeps feature maps across forwards; there is no cached form of the "
                             "sampled forward")
        if self.estimator.dropout <= 0:
            raise ValueError("estimate_samples samples PSPNet's Dropout2d, which this estimator runs without: it needs cfg hip_dropout > 0 "
                             "or hip_as_shipped: true (every sample would be the same box otherwise)")
        if self.prepare_mode != "device":
            raise ValueError(f'estimate_samples crops on the device: it needs hip_prepare: "device", got {self.prepare_mode!r}')
        S = int(samples)
        if not 1 <= S <= samples_mod.MAX_SAMPLES or S != samples:
            raise ValueError(f"estimate_samples: samples must be an integer in 1 .. {samples_mod.MAX_SAMPLES}, got {samples!r}")
        return S

    def estimate_samples(self, camera_intrinsic_batch, rgb1_batch, view1_mask_batch, view1_extrinsic_batch, rgb2_batch, view2_mask_batch,
                         view2_extrinsic_batch, samples: int = 8, select=None):
        """`estimate` (same arguments, frame types and hip_upload modes) drawing `samples` = S Dropout2d samples of every pose instead of
        one, and what they say about the box, as a dict of numpy arrays.  The frames are uploaded and cropped once and the `choose`
        subsets drawn once; `AdaPoseNet.forward_samples` runs the backbone in front of the first Dropout2d site once per pose and the
        rest once per sample; the configured box tail (median, v4's regressed, RANSAC or PnP) runs on the S n rows as one batch of S n
        poses (a seeded tail sees pose index s n + i).  Returns `bbox` [n,8,3] f64 (the mean box over the counted samples, the +10 cube
        where none counts), `bbox_samples` [n,S,8,3] f64, `count` [n] i32, `bbox_std` [n,8,3], `center_cov` [n,3,3], `extent_mean` /
        `extent_std` [n,3] (edges x, y, z of the box frame), `axis_spread_deg` [n,3] (all f64, `samples.box_stats`), `nocs_mean` /
        `nocs_std` [n,1024,3] and `depth_mean` / `depth_std` [n,1024] f32 of the view-1 point outputs (`samples.point_stats`; NaN for a
        pose with an empty mask) and `valid` [n] i32 (count > 0).  A sample counts if its pose was valid at prepare, its tail did not
        return the +10 cube and its box is finite.  Poses are processed in chunks of at most 256 // S, each chunk one `forward_samples`:
        the mask sequence is therefore per chunk (pose i of a chunk starting at pose c, sample s, draws global pose index
        counter + s m + (i - c), m the poses of the chunk; the counter advances by S m per chunk).  Needs cfg hip_dropout > 0 or
        hip_as_shipped, no hip_feature_cache, hip_prepare: "device" and 1 <= samples <= 64.  `select="mask"`: the S draws and the mean
        box (hypothesis S) are scored against the two frame masks (`verify.samples_verify`) and the dict gains `bbox_best` [n,8,3] f64
        (the hypothesis with the largest mean mask IoU, the +10 cube where none is usable), `best` [n] i64 (its index, -1 for none),
        `mask_score` [n,S+1] and `mask_iou` [n,S+1,2] f64; the masks are the ones uploaded for the crops (hip_upload: "windows", which
        uploads crop windows only: one upload of the uint8 masks).  Any other `select` but None is refused."""
        S = self._samples_check(samples, select)
        n = len(rgb1_batch)
        dev = self.estimator.device
        Kd = torch.as_tensor(np.asarray(camera_intrinsic_batch)).to(dev)
        args = (rgb1_batch, rgb2_batch, view1_mask_batch, view2_mask_batch)
        cuda = [isinstance(x, torch.Tensor) and x.is_cuda for x in args]
        wp = self._pnp_branch()
        size = self.cfg["img_size"]
        if self.upload_mode == "windows" and not any(cuda):
            srcs = [host_array(x) for x in args]
            ring = self._wring = WindowRing.matching(self._wring, n, srcs, dev, slots=1, grow=True)
            ring.payload_bytes = ring.table_bytes = 0
            ring.wait(0)
            ring.stage(0, srcs, 0, n)
            d = ring.copy(0, n)
            a, b = (self._prepare_windows(d, v, Kd, size, 1024, self.prepare_seed + v, want_pts2d=wp) for v in (0, 1))
            self.upload_bytes_last_call, self.upload_table_bytes_last_call = ring.payload_bytes, ring.table_bytes
            m1, m2 = (self._upload_masks(view1_mask_batch), self._upload_masks(view2_mask_batch)) if select else (None, None)
        else:
            self.upload_bytes_last_call, self.upload_table_bytes_last_call = frames_payload_bytes(*args), 0
            m1, m2 = self._upload_masks(view1_mask_batch), self._upload_masks(view2_mask_batch)
            a = self._prepare(self._upload_frames(rgb1_batch), m1, Kd, size, 1024, self.prepare_seed, want_pts2d=wp)
            b = self._prepare(self._upload_frames(rgb2_batch), m2, Kd, size, 1024, self.prepare_seed + 1, want_pts2d=wp)
        E1, E2 = np.asarray(view1_extrinsic_batch), np.asarray(view2_extrinsic_batch)
        return _to_host(self._samples_selected(self._samples_prepared(a, b, E1, E2, Kd, S), select, Kd, E1, m1, E2, m2))

    def estimate_samples_device(self, K, rgb1, mask1, E1, rgb2, mask2, E2, samples: int = 8, frame0: int = 0, select=None):
        """`estimate_samples` for frames that live on the GPU (the arguments of `estimate_device`): the same dict, as CUDA tensors."""
        S = self._samples_check(samples, select)
        size, dev = self.cfg["img_size"], self.estimator.device
        Kd = torch.as_tensor(K).to(dev)
        kw = dict(want_pts2d=self._pnp_branch(), frame0=frame0)
        m1, m2 = torch.as_tensor(mask1).to(dev), torch.as_tensor(mask2).to(dev)
        a = self._prepare(torch.as_tensor(rgb1).to(dev), m1, Kd, size, 1024, self.prepare_seed, **kw)
        b = self._prepare(torch.as_tensor(rgb2).to(dev), m2, Kd, size, 1024, self.prepare_seed + 1, **kw)
        return self._samples_selected(self._samples_prepared(a, b, E1, E2, Kd, S), select, Kd, E1, m1, E2, m2)

    @staticmethod
    def _samples_selected(res, select, K, E1, mask1, E2, mask2):
        """The result of `_samples_prepared` (CUDA tensors), with the keys of `select="mask"` where that is asked for."""
        if select is None:
            return res
        v = verify_mod.samples_verify(res, K, E1, mask1, E2, mask2)
        res.update(bbox_best=v["bbox_best"], best=v["best"], mask_score=v["score"], mask_iou=v["iou"])
        return res

    def _samples_prepared(self, a, b, E1, E2, K, S: int):
        """The sampled network, the box tail on the S n rows and the statistics, for the prepared views a / b."""
        dev = self.estimator.device
        E1d = torch.as_tensor(E1).to(device=dev, dtype=torch.float64)
        E2d = torch.as_tensor(E2).to(device=dev, dtype=torch.float64)
        n = int(E1d.shape[0])
        depths = self._consts(dev)[1][None].expand(n, 24).contiguous()
        P1, P2 = self._projection(a["Kcrop"], E1d), self._projection(b["Kcrop"], E2d)
        chunk = max(self._SAMPLE_ROWS // S, 1)
        pred = None
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            part = self.estimator.forward_samples(a["img"][lo:hi], a["choose"][lo:hi], b["img"][lo:hi], b["choose"][lo:hi], P1[lo:hi], P2[lo:hi],
                                                  depths[lo:hi], samples=S)
            self._plain_views += 2 * (hi - lo)
            if hi - lo == n:
                pred = part
                break
            if pred is None:
                pred = {k: torch.empty(S, n, *v.shape[2:], dtype=v.dtype, device=dev) for k, v in part.items()}
            for k, v in part.items():
                pred[k][:, lo:hi] = v
        rows = {k: v.reshape(S * n, *v.shape[2:]) for k, v in pred.items()}                # row s n + i
        tile = lambda t: None if t is None else torch.as_tensor(t).to(dev).repeat(S, *([1] * (t.dim() - 1)))      # noqa: E731
        bbox = self._bbox_tail(rows, tile(a["choose"]), tile(a["Kcrop"]), tile(E1d), pts2d=(tile(a.get("pts2d")), tile(b.get("pts2d"))),
                               E2=tile(E2d), K=tile(torch.as_tensor(K)))
        dflt = self._consts(dev)[0]
        prepared = (a["valid"] != 0) & (b["valid"] != 0)
        ok = prepared.repeat(S) & ~(bbox == dflt).all(dim=2).all(dim=1)
        box = torch.where(prepared.repeat(S).view(S * n, 1, 1), bbox, dflt.expand(S * n, 8, 3)).view(S, n, 8, 3)
        st = samples_mod.box_stats(box, ok.view(S, n))
        counted = st["count"] > 0
        nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        res = {"bbox": torch.where(counted.view(n, 1, 1), st["bbox_mean"], dflt.expand(n, 8, 3)), "bbox_samples": box.transpose(0, 1).contiguous(),
               "count": st["count"], "valid": counted.to(torch.int32)}
        res.update({k: st[k] for k in ("bbox_std", "center_cov", "extent_mean", "extent_std", "axis_spread_deg")})
        for key, src in (("nocs", "view1_nocs"), ("depth", "view1_depth")):
            mean, std = samples_mod.point_stats(pred[src])
            keep = prepared.view(n, *([1] * (mean.dim() - 1)))
            res[f"{key}_mean"], res[f"{key}_std"] = torch.where(keep, mean, nan), torch.where(keep, std, nan)
        return res


class AdaPoseEstimator_v4(AdaPoseEstimator_v5):
    """`pose_estimator.name: adapose_v4` (`interface_v4.py:37-378`): the constructor, call surface and `hip_*` keys of
    `AdaPoseEstimator_v5` on the same network and checkpoint; upload, device / host prepare, 8-bit frames, the feature caches and the
    `direct_regression: False` tails are the code above."""

    @property
    def _normalize(self) -> bool:
        """interface_v4.py:52-58: ToTensor + ImageNet Normalize for task "pots", plain ToTensor (the crop itself) for every other task."""
        return self.cfg["task_name"] == "pots"

    def _regressed_tail(self, pred, choose, Kcrop, E1):
        """interface_v4.py:322-325: tt = view1_t, ts = ||view1_s|| — the network's own heads, no pair median."""
        return postprocess_regressed(pred["view1_nocs"], pred["view1_r"], pred["view1_t"], pred["view1_s"], E1)[0]


class AdaPoseEstimator_baseline(AdaPoseEstimator_v5):
    """`pose_estimator.name: adapose_baseline` (`interface_baseline.py`, which is `interface_v5.py` with the network class changed):
    `StereoPoseNet_with_depth_baseline(regress_pose=cfg["direct_regression"])` — v5's PSPNet and point heads, the plane-sweep cost
    volume replaced by attention between the two views' chosen points.  Crop, upload, 8-bit frames, windows, the
    three box tails and `hip_dtype` / `hip_prepare` / `hip_upload` / `hip_view2_heads` / `hip_options` are the code above.  What reads the
    cost volume or is not implemented for this network raises, naming the key."""

    _UNSUPPORTED = ("hip_feature_cache", "hip_dropout", "hip_as_shipped", "hip_graph")

    def __init__(self, env, cfg, logger, state_dict=None, dtype=None, device=0, net=None):
        for key in self._UNSUPPORTED:
            if cfg.get(key, False):
                raise ValueError(f"AdaPoseEstimator_baseline: cfg key {key} is not implemented for the baseline network")
        if cfg.get("hip_norm_mode", "eval") not in ("eval", 0):
            raise ValueError("AdaPoseEstimator_baseline: cfg key hip_norm_mode: the baseline network has no BatchNorm3d")
        if net is not None and getattr(net, "arch", "v5") != "baseline":
            raise ValueError("AdaPoseEstimator_baseline: the shared net must be an AdaPoseNet(arch='baseline')")
        super().__init__(env, cfg, logger, state_dict=state_dict, dtype=dtype, device=device, net=net)

    def _synthetic_state_dict(self):
        from . import synth
        return synth.baseline_state_dict(seed=0, regress_pose=bool(self.cfg["direct_regression"]))

    def _build_net(self, state_dict, device, norm_mode, drop_p, drop_seed, options):
        return AdaPoseNet(state_dict, dtype=self.dtype, device=device, options=options, arch="baseline",
                          regress_pose=bool(self.cfg["direct_regression"]))

    def _no_cost_volume(self, name):
        raise NotImplementedError(f"AdaPoseEstimator_baseline.{name}: the dense maps come from the cost volume, which the baseline network "
                                  "does not have")

    def estimate_samples(self, *a, **k):
        raise NotImplementedError("AdaPoseEstimator_baseline.estimate_samples: Dropout2d (cfg hip_dropout / hip_as_shipped) is not implemented "
                                  "for the baseline network, so there is nothing to sample")

    def estimate_samples_device(self, *a, **k):
        raise NotImplementedError("AdaPoseEstimator_baseline.estimate_samples_device: Dropout2d (cfg hip_dropout / hip_as_shipped) is not "
                                  "implemented for the baseline network, so there is nothing to sample")

    def estimate_depth(self, *a, **k):
        self._no_cost_volume("estimate_depth")

    def estimate_depth_device(self, *a, **k):
        self._no_cost_volume("estimate_depth_device")

    def estimate_cloud(self, *a, **k):
        self._no_cost_volume("estimate_cloud")

    def estimate_cloud_device(self, *a, **k):
        self._no_cost_volume("estimate_cloud_device")

    def estimate_cloud_pose(self, *a, **k):
        self._no_cost_volume("estimate_cloud_pose")

    def estimate_cloud_pose_device(self, *a, **k):
        self._no_cost_volume("estimate_cloud_pose_device")

    def estimate_cloud_views(self, *a, **k):
        self._no_cost_volume("estimate_cloud_views")

    def estimate_cloud_views_device(self, *a, **k):
        self._no_cost_volume("estimate_cloud_views_device")


class AdaPoseEstimator_realworld(AdaPoseEstimator_v5):
    """`pose_estimator.name: adapose_realworld` (`interface_realworld.py`, whose `prepare_model_input` / `estimate` are `interface_v5.py`'s):
    `StereoPoseNet_with_depth_for_realdemo` - v5 on a variance cost volume with the pose rows read from camera points (DESIGN.md section
    5r) - and the PnP tail with the regressed size (`interface_realworld.py:295-320`, csrc/pnp.hip: pnp_scaled_kernel), which reads
    view 1's NOCS and size only: `hip_view2_heads` defaults to False whatever `direct_regression` / `use_depth` say (the tail has no
    such branches).  Crop, upload, 8-bit frames, windows and `hip_dtype` (not fp16) / `hip_upload` / `hip_options` are the code above.
    One deliberate difference from the shipped interface: its line 287 calls the network with seven arguments where `forward` takes nine
    and never passes the coordinates it computes at :264-269 (`predict` raises TypeError as shipped); this class passes them.  What is
    not implemented for this network raises, naming the key."""

    _UNSUPPORTED = ("hip_feature_cache", "hip_dropout", "hip_as_shipped", "hip_graph")

    def __init__(self, env, cfg, logger, state_dict=None, dtype=None, device=0, net=None):
        for key in self._UNSUPPORTED:
            if cfg.get(key, False):
                raise ValueError(f"AdaPoseEstimator_realworld: cfg key {key} is not implemented for the real-world network")
        if cfg.get("hip_norm_mode", "eval") not in ("eval", 0):
            raise ValueError("AdaPoseEstimator_realworld: cfg key hip_norm_mode: per-sample BatchNorm3d is not implemented for the real-world network")
        if cfg.get("hip_prepare", "device") != "device":
            raise ValueError('AdaPoseEstimator_realworld: cfg key hip_prepare: only "device" is implemented for the real-world network')
        if (dtype or cfg.get("hip_dtype", "bf16x3")) in ("fp16", "f16", "float16"):
            raise ValueError("AdaPoseEstimator_realworld: cfg key hip_dtype: fp16 is not implemented for the real-world network (a voxel of its "
                             "variance volume is a product of two feature values; f16 saturates at 65504): use bf16x3, bf16 or fp32")
        if net is not None and getattr(net, "arch", "v5") != "realworld":
            raise ValueError("AdaPoseEstimator_realworld: the shared net must be an AdaPoseNet(arch='realworld')")
        super().__init__(env, cfg, logger, state_dict=state_dict, dtype=dtype, device=device, net=net)

    def _synthetic_state_dict(self):
        from . import synth
        return synth.realworld_state_dict(seed=0)

    def _build_net(self, state_dict, device, norm_mode, drop_p, drop_seed, options):
        return AdaPoseNet(state_dict, dtype=self.dtype, device=device, options=options, arch="realworld")

    def _pnp_branch(self):
        """No `direct_regression` / `use_depth` branches here: the one tail reads view 1 alone (the view-2 heads are not needed)."""
        return False

    # the pixels of the chosen points are always wanted: the network reads them normalised, the tail as they are
    def _prepare(self, rgb, *args, **kw):
        out = super()._prepare(rgb, *args, **{**kw, "want_pts2d": True})
        out["coor"] = pts2d_to_coor(out["pts2d"], W=int(rgb.shape[2]), H=int(rgb.shape[1]))
        return out

    def _prepare_windows(self, d, v, K, *args, **kw):
        out = super()._prepare_windows(d, v, K, *args, **{**kw, "want_pts2d": True})
        out["coor"] = pts2d_to_coor(out["pts2d"], W=int(d.W), H=int(d.H))
        return out

    def _network_inputs(self, a, b) -> dict:
        return {"coor1": a["coor"], "coor2": b["coor"]}

    def _bbox_tail(self, pred, choose, Kcrop, E1, pts2d=None, E2=None, K=None):
        """interface_realworld.py:295-320: ts = ||view1_s||, EPnP-RANSAC + VVS on (nocs1 ts, pixels of view 1, the ORIGINAL intrinsics)."""
        return postprocess_pnp_scaled(pred["view1_nocs"], pts2d[0], pred["view1_s"], K, E1, seed=int(self.cfg.get("hip_ransac_seed", 0)))[0]

    def _refused(self, name, why):
        raise NotImplementedError(f"AdaPoseEstimator_realworld.{name}: {why} is not implemented for the real-world network")

    def estimate_samples(self, *a, **k):
        self._refused("estimate_samples", "Dropout2d (cfg hip_dropout / hip_as_shipped), so there is nothing to sample,")

    def estimate_samples_device(self, *a, **k):
        self._refused("estimate_samples_device", "Dropout2d (cfg hip_dropout / hip_as_shipped), so there is nothing to sample,")

    def estimate_depth(self, *a, **k):
        self._refused("estimate_depth", "the dense forward")

    def estimate_depth_device(self, *a, **k):
        self._refused("estimate_depth_device", "the dense forward")

    def estimate_cloud(self, *a, **k):
        self._refused("estimate_cloud", "the dense forward")

    def estimate_cloud_device(self, *a, **k):
        self._refused("estimate_cloud_device", "the dense forward")

    def estimate_cloud_pose(self, *a, **k):
        self._refused("estimate_cloud_pose", "the dense forward")

    def estimate_cloud_pose_device(self, *a, **k):
        self._refused("estimate_cloud_pose_device", "the dense forward")

    def estimate_cloud_views(self, *a, **k):
        self._refused("estimate_cloud_views", "the dense forward")

    def estimate_cloud_views_device(self, *a, **k):
        self._refused("estimate_cloud_views_device", "the dense forward")


class AdaPoseEstimator_v2(AdaPoseEstimator_v5):
    """`pose_estimator.name: adapose_v2` (`interface_v2.py`): `StereoPoseNet` - v5's PSPNet and NOCS branch, a pointwise stereo part
    evaluated at the chosen pixels and a size branch, no depth, rotation or translation - behind a
    `prepare_model_input` that draws the 1024 points from the frame mask at native resolution and maps them into the crop afterwards
    (`interface_v2.py:74-98`; `prepare_inputs(sample="native")`), and the PnP tail with the regressed size (`interface_v2.py:242-266`,
    csrc/pnp.hip: pnp_scaled_kernel), which reads view 1's NOCS, pixels and size only: `hip_view2_heads` defaults to False, and
    `use_depth` / `direct_regression` are not read, as in the reference.  `hip_dtype` (all four) and `hip_options` are the code above.
    One deliberate difference from the shipped interface: its line 239 calls `depth_estimation_from_nocs_matches` with 7 arguments where
    `lib/utils.py:121` takes 9, so `predict` raises TypeError as shipped; the call's result is unused there, and it is not made here.
    What is not implemented for this network raises, naming the key."""

    _UNSUPPORTED = ("hip_feature_cache", "hip_dropout", "hip_as_shipped", "hip_graph")
    _ARCH = "v2"      # the AdaPoseNet arch behind this class and the name its messages carry (AdaPoseEstimator_v1 overrides it)

    def __init__(self, env, cfg, logger, state_dict=None, dtype=None, device=0, net=None):
        arch, who = self._ARCH, "AdaPoseEstimator_" + self._ARCH
        for key in self._UNSUPPORTED:
            if cfg.get(key, False):
                raise ValueError(f"{who}: cfg key {key} is not implemented for the {arch} network")
        if cfg.get("hip_norm_mode", "eval") not in ("eval", 0):
            raise ValueError(f"{who}: cfg key hip_norm_mode: per-sample BatchNorm3d is not implemented for the {arch} network (it would "
                             "need the whole volume, which this network's kernel never builds)")
        if cfg.get("hip_prepare", "device") != "device":
            raise ValueError(f'{who}: cfg key hip_prepare: only "device" is implemented for the {arch} network')
        if cfg.get("hip_upload", "frames") != "frames":
            raise ValueError(f'{who}: cfg key hip_upload: only "frames" is implemented for the {arch} network (the points are drawn '
                             "from the whole frame's mask)")
        if net is not None and getattr(net, "arch", "v5") != arch:
            raise ValueError(f"{who}: the shared net must be an AdaPoseNet(arch='{arch}')")
        super().__init__(env, cfg, logger, state_dict=state_dict, dtype=dtype, device=device, net=net)

    def _synthetic_state_dict(self):
        from . import synth
        return synth.v2_state_dict(seed=0)

    def _build_net(self, state_dict, device, norm_mode, drop_p, drop_seed, options):
        return AdaPoseNet(state_dict, dtype=self.dtype, device=device, options=options, arch="v2")

    def _pnp_branch(self):
        """No `direct_regression` / `use_depth` branches here: the one tail reads view 1 alone (the view-2 heads are not needed)."""
        return False

    # the points are drawn at native resolution, and their pixels are always wanted: the tail reads them
    def _prepare(self, rgb, *args, **kw):
        return super()._prepare(rgb, *args, **{**kw, "want_pts2d": True, "sample": "native"})

    def _bbox_tail(self, pred, choose, Kcrop, E1, pts2d=None, E2=None, K=None):
        """interface_v2.py:242-266: ts = ||view1_s||, EPnP-RANSAC + VVS on (nocs1 ts, pixels of view 1, the ORIGINAL intrinsics)."""
        return postprocess_pnp_scaled(pred["view1_nocs"], pts2d[0], pred["view1_s"], K, E1, seed=int(self.cfg.get("hip_ransac_seed", 0)))[0]

    def _refused(self, name, why):
        raise NotImplementedError(f"AdaPoseEstimator_{self._ARCH}.{name}: {why} is not implemented for the {self._ARCH} network")

    def estimate_samples(self, *a, **k):
        self._refused("estimate_samples", "Dropout2d (cfg hip_dropout / hip_as_shipped), so there is nothing to sample,")

    def estimate_samples_device(self, *a, **k):
        self._refused("estimate_samples_device", "Dropout2d (cfg hip_dropout / hip_as_shipped), so there is nothing to sample,")

    def estimate_depth(self, *a, **k):
        self._refused("estimate_depth", "the dense forward")

    def estimate_depth_device(self, *a, **k):
        self._refused("estimate_depth_device", "the dense forward")

    def estimate_cloud(self, *a, **k):
        self._refused("estimate_cloud", "the dense forward")

    def estimate_cloud_device(self, *a, **k):
        self._refused("estimate_cloud_device", "the dense forward")

    def estimate_cloud_pose(self, *a, **k):
        self._refused("estimate_cloud_pose", "the dense forward")

    def estimate_cloud_pose_device(self, *a, **k):
        self._refused("estimate_cloud_pose_device", "the dense forward")

    def estimate_cloud_views(self, *a, **k):
        self._refused("estimate_cloud_views", "the dense forward")

    def estimate_cloud_views_device(self, *a, **k):
        self._refused("estimate_cloud_views_device", "the dense forward")


class AdaPoseEstimator_v1(AdaPoseEstimator_v2):
    """`pose_estimator.name: adapose` (`interface.py`, `train.py:222-224`): the v1 `StereoPoseNet` (lib/network.py)
    behind the code of `AdaPoseEstimator_v2` - `interface.py` equals `interface_v2.py` line for line apart from the class name and the
    network import: the points drawn at native resolution, the PnP tail scaled by the regressed size, the unused helper call that is not
    made.  The network also regresses r and t for both views; the tail reads view 1's NOCS, pixels and size only, so `hip_view2_heads`
    defaults to False here too.  The same cfg keys are refused, under this class's name."""

    _ARCH = "v1"

    def _synthetic_state_dict(self):
        from . import synth
        return synth.v1_state_dict(seed=0)

    def _build_net(self, state_dict, device, norm_mode, drop_p, drop_seed, options):
        return AdaPoseNet(state_dict, dtype=self.dtype, device=device, options=options, arch="v1")

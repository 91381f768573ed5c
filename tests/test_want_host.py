"""CPU-only checks of the result plan of the two-view estimator calls (`estimator.ResultPlan`, passed as `want=`): what a pipelined call's
chunks are written into is, key for key, what the docstrings of `estimate`, `estimate_depth`, `estimate_cloud` and `estimate_cloud_pose`
promise; the keywords each kind adds to the prepare and network calls; and `adapose` still exports the geometry ops that moved to
`cloud`."""
import dataclasses
import types

import pytest
import torch

from rgbmanip_amd import adapose, cloud
from rgbmanip_amd.config import ADAPOSE_CFGS
from rgbmanip_amd.estimator import BOXES, AdaPoseEstimator_v5, ResultPlan

N, S, CAP = 3, 8, 5
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
DEPTH = {"bbox": (F64, (N, 8, 3)), "depth": (F32, (N, S, S)), "conf": (F32, (N, S, S)), "points": (F32, (N, S, S, 3)), "window": (I32, (N, 4)),
         "Kcrop": (F64, (N, 3, 3)), "valid": (I32, (N,))}
CLOUD = dict(DEPTH, depth2=(F32, (N, S, S)), conf2=(F32, (N, S, S)), window2=(I32, (N, 4)), Kcrop2=(F64, (N, 3, 3)), mask1=(U8, (N, S, S)),
             mask2=(U8, (N, S, S)), cloud=(F32, (N, CAP, 3)), cloud_index=(I32, (N, CAP)), count=(I32, (N, 2)),
             **{f"{k}{v}": (U8 if k == "keep" else F32, (N, S, S)) for k in ("fused", "keep", "reproj", "rel") for v in (1, 2)})
POSE = dict(CLOUD, nocs1=(F32, (N, S, S, 3)), nocs2=(F32, (N, S, S, 3)), cloud_nocs=(F32, (N, CAP, 3)))
KINDS = {"depth": (ResultPlan(maps=True), DEPTH, {}, {"dense_depth": True}),
         "cloud": (ResultPlan(True, True, cap=CAP), CLOUD, {"want_mask": True}, {"dense_depth": True}),
         "cloud_pose": (ResultPlan(True, True, cap=CAP, fit_seed=0), POSE, {"want_mask": True}, {"dense_depth": True, "dense_nocs": True})}


def _est():
    net = types.SimpleNamespace(options={"view2_heads": 1}, dropout=0.0, dropout_seed=0, device="cpu", feature_bytes=64)
    return AdaPoseEstimator_v5(None, dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, img_size=S, hip_view2_heads=True), None, net=net)


def test_boxes_plan():
    assert BOXES == ResultPlan() and BOXES.prepare_kw == {} and BOXES.network_kw == {}
    assert not BOXES.maps and not BOXES.cloud and not BOXES.fit
    out = _est()._alloc_out(n=N, dev="cpu", want=BOXES)
    assert isinstance(out, torch.Tensor) and out.dtype == F64 and tuple(out.shape) == (N, 8, 3)


@pytest.mark.parametrize("kind", list(KINDS))
def test_chunk_outputs_and_keywords(kind):
    want, promised, prepare_kw, network_kw = KINDS[kind]
    out = _est()._alloc_out(n=N, dev="cpu", want=want)
    assert set(out) == set(promised)
    for k, (dtype, shape) in promised.items():
        assert out[k].dtype == dtype and tuple(out[k].shape) == shape, k
    for k in ("bbox_cloud", "srt_cloud", "fit_info", "valid_cloud"):      # added after the chunks, over the whole call
        assert k not in out
    assert want.prepare_kw == prepare_kw and want.network_kw == network_kw
    assert want.maps and want.cloud == (kind != "depth") and want.fit == (kind == "cloud_pose")


def test_cloud_options_build_the_plan():
    est = _est()
    want = est._cloud_options(2.0, 0.02, 0.5, False, CAP)
    assert want == ResultPlan(True, True, 2.0, 0.02, 0.5, False, CAP, None)
    assert est._cloud_options(1.0, 0.01, 0.0, True, None).cap == 2 * S * S
    assert est._cloud_options(1.0, 0.01, 0.0, True, CAP, fit_seed=0).fit      # seed 0 is a seed
    with pytest.raises(dataclasses.FrozenInstanceError):
        want.cap = 1                                                      # frozen


MOVED = ("depth_to_points", "depth_to_points_ref", "depth_consistency", "depth_consistency_ref", "depth_fusion", "depth_fusion_ref",
         "cloud_pack", "cloud_pack_views", "cloud_gather", "cloud_gather_views", "cloud_similarity", "cloud_similarity_ref")


@pytest.mark.parametrize("name", MOVED)
def test_adapose_reexports_the_moved_ops(name):
    assert getattr(adapose, name) is getattr(cloud, name)

"""Every output array of a fixed list of AdaPoseNet calls on the golden inputs and seeded weights, written to an .npz: run it in two trees
(each run its own process with its own built librgbm_hip.so) and compare bit for bit.

usage: ab_forward_outputs.py out.npz            (in each tree)
       ab_forward_outputs.py --compare a.npz b.npz

Only the Python names both trees have are used.  Arrays are compared as bytes (view2_heads = 0 fills the view-2 outputs with NaN).
Besides the forwards of the v5 and the baseline network the list holds the 3-D taps of a dense cost regularisation (element count and
SHA-256 each), and under "sizes" the node counts of the captured graphs, workspace_bytes(B) for B = 1, 2, 3, 256 and feature_bytes
(the baseline network has no feature cache, so only its workspace sizes are listed).  The path-selection block runs every option value
and debug flag that moves a decision of the forward (csrc/forward_paths.cpp) once: B = 2 plain and dense, the captured B = 1 forward, and
under "sizes" that configuration's workspace, dense-workspace and feature sizes and node count; an fp16 net, forward_samples at S = 2."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    if sorted(A.files) != sorted(B.files):
        print("different call lists:", sorted(set(A.files) ^ set(B.files)))
        return 1
    for k in A.files:
        if A[k].shape != B[k].shape or A[k].dtype != B[k].dtype or A[k].tobytes() != B[k].tobytes():
            print(f"FIRST DIFFERENCE at {k}: shapes {A[k].shape} {B[k].shape}")
            return 1
    calls = sorted({k.rsplit(" | ", 1)[0] for k in A.files})
    print(f"all equal: {len(A.files)} arrays of {len(calls)} calls\n" + "\n".join(calls))
    return 0


def main(path):
    import torch
    from rgbmanip_amd import synth
    from rgbmanip_amd.adapose import AdaPoseNet
    out, sizes = {}, {}
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    inputs = {B: synth.adapose_inputs(B, seed=0) for B in (1, 2, 4)}      # B = 2: the batch of tests/golden/adapose_b2*.npz

    def put(name, pred):
        torch.cuda.synchronize()
        print(name, flush=True)
        for k, v in pred.items():
            out[f"{name} | {k}"] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    def call(net, B, **kw):
        i = inputs[B]
        return net(i["img1"], i["choose1"], i["img2"], i["choose2"], i["P1"], i["P2"], i["depths"], **kw)

    variants = (("plain", {}), ("dense_depth", dict(dense_depth=True)), ("dense_nocs", dict(dense_nocs=True)),
                ("dense_depth+dense_nocs", dict(dense_depth=True, dense_nocs=True)))
    for dt in ("bf16", "bf16x3", "fp32"):
        for v2h in (1, 0):
            net = AdaPoseNet(sd, dtype=dt, max_chunk_views=2, options={"view2_heads": v2h})
            for B in (1, 2):
                for vn, kw in variants:
                    put(f"{dt} view2_heads={v2h} B={B} {vn}", call(net, B, **kw))
                put(f"{dt} view2_heads={v2h} B={B} plain again", call(net, B))
            # the forward split at the PSPNet's output
            i = inputs[2]
            pool = net.feature_pool(4)
            net.features(np.concatenate([i["img1"], i["img2"]]), np.arange(4), pool)
            put(f"{dt} view2_heads={v2h} B=2 features + forward_cached",
                net.forward_cached(pool, [0, 1], [2, 3], i["choose1"], i["choose2"], i["P1"], i["P2"], i["depths"]))
        net = AdaPoseNet(sd, dtype=dt, graph=True)
        for rep in range(3):
            put(f"{dt} graph B=1 run {rep}", call(net, 1))
    net = AdaPoseNet(sd, dtype="bf16", split_streams=True, split_min_batch=4)
    for rep in range(2):
        put(f"bf16 split_streams B=4 run {rep}", call(net, 4))
    # the K-split launches (B = 1 per stream) on two side streams of one net, and on a net created behind a destroyed one
    net = AdaPoseNet(sd, dtype="bf16", split_streams=True, split_min_batch=2)
    for rep in range(2):
        put(f"bf16 split_streams B=2 run {rep}", call(net, 2))
    on_device = [torch.as_tensor(inputs[1][k]).cuda().to(torch.int32 if k.startswith("choose") else torch.float32).contiguous()
                 for k in ("img1", "choose1", "img2", "choose2", "P1", "P2", "depths")]
    torch.cuda.synchronize()      # the side stream below reads them
    for rep in range(2):
        net = AdaPoseNet(sd, dtype="bf16")
        put(f"bf16 B=1 on a fresh stream, net {rep} (the one before it destroyed)", net(*on_device, stream=torch.cuda.Stream()))
        net.close()
    # Dropout2d: drawn masks (two eager forwards; capture + two replays), then explicit masks, then the sequence goes on
    for graph in (False, True):
        net = AdaPoseNet(sd, dtype="bf16", dropout=0.1, dropout_seed=3, graph=graph)
        for rep in range(3 if graph else 2):
            put(f"bf16 dropout 0.1 seed 3 graph={graph} B=2 run {rep}", call(net, 2))
            put(f"bf16 dropout 0.1 seed 3 graph={graph} B=2 run {rep} masks", {"masks": net.dropout_masks(2)})
        masks = (np.random.default_rng(7).random((4, 320)) > 0.1).astype(np.float32) / np.float32(0.9)
        net.set_dropout_masks(masks)
        put(f"bf16 dropout graph={graph} explicit masks B=2", call(net, 2))
        put(f"bf16 dropout graph={graph} explicit masks B=2 masks", {"masks": net.dropout_masks(2)})
        put(f"bf16 dropout graph={graph} after explicit masks B=2", call(net, 2))
        put(f"bf16 dropout graph={graph} after explicit masks B=2 masks", {"masks": net.dropout_masks(2)})
    net = AdaPoseNet(sd, dtype="bf16")
    net.set_dropout_masks(masks)
    put("bf16 explicit masks on a net without dropout B=2", call(net, 2, dense_depth=True))
    put("bf16 explicit masks on a net without dropout B=2, next forward", call(net, 2))
    # the other chunk bodies of cost_volume(), two chunks each
    for name, dt, kw in (("norm_mode=1", "fp32", dict(norm_mode=1)), ("norm_mode=1", "bf16x3", dict(norm_mode=1)), ("cost_impl=0", "bf16", dict(cost_impl=0)),
                         ("cost_impl=1", "bf16", dict(cost_impl=1)), ("cost_impl=2", "bf16", dict(cost_impl=2)), ("cost_impl=2", "fp32", dict(cost_impl=2))):
        net = AdaPoseNet(sd, dtype=dt, max_chunk_views=2, **kw)
        put(f"{dt} {name} B=2 plain", call(net, 2))
        put(f"{dt} {name} B=2 dense_depth", call(net, 2, dense_depth=True))
    # stop_after through the taps it leaves behind
    for dt in ("bf16", "bf16x3"):
        net = AdaPoseNet(sd, dtype=dt)
        call(net, 2, stop_after=1)
        put(f"{dt} stop_after=1 B=2", {"feat": net.fetch(2, "feat", 4 * 224 * 224 * 32), "layer4": net.fetch(2, "layer4", 4 * 28 * 28 * 512)})
        call(net, 2, stop_after=2)
        put(f"{dt} stop_after=2 B=2", {"prob": net.fetch(2, "prob", 4 * 1024 * 24)})
    # the baseline network (no cost volume): two chunks of poses
    for dt in ("bf16", "fp32"):
        for rp in (True, False):
            bsd = synth.baseline_state_dict(seed=0, regress_pose=rp)
            for v2h in ((1, 0) if dt == "bf16" else (1,)):
                net = AdaPoseNet(bsd, dtype=dt, arch="baseline", regress_pose=rp, max_chunk_views=2, options={"view2_heads": v2h})
                put(f"{dt} baseline regress_pose={rp} view2_heads={v2h} B=2", call(net, 2))
                sizes[f"baseline {dt} regress_pose={rp} view2_heads={v2h}"] = [net.workspace_bytes(B) for B in (1, 2, 3, 256)]
    # the 3-D taps of a dense cost regularisation, B = 1: element count and SHA-256 of the bytes (c0 alone is 77 MB)
    for dt in ("bf16", "fp32"):
        for taps, kw in ((("c0", "c2", "c4", "c6", "u7", "u9"), {}), (("u11",), dict(sparse_tail=0))):
            net = AdaPoseNet(sd, dtype=dt, options={"sparse_dec": 0}, **kw)
            call(net, 1)
            torch.cuda.synchronize()
            for t in taps:
                a = net.fetch(1, t, 2 * 24 * 224 * 224 * 8).cpu().numpy()
                put(f"{dt} sparse_dec=0 B=1 tap {t}", {"count": a.size, "sha256": np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)})
    # path selection: every option value and debug flag that moves a decision of the forward, once each at B = 2 (eager), with the sizes
    # the configuration asks for and the node count of its captured B = 1 forward
    from rgbmanip_amd import _lib
    lib = _lib.load()

    def config(name, dt, flags=0, state=sd, **kw):
        _lib.check(lib.rgbm_debug_flags(flags), "rgbm_debug_flags")
        try:
            net = AdaPoseNet(state, dtype=dt, **kw)
            put(f"{name} B=2", call(net, 2))
            sz = [net.workspace_bytes(1), net.workspace_bytes(2), net.workspace_bytes(256)]
            if net.arch == "v5":      # the baseline network has neither dense calls, a feature cache nor graph replay
                put(f"{name} B=2 dense_depth", call(net, 2, dense_depth=True))
                sz += [net.dense_workspace_bytes(1), net.dense_workspace_bytes(2), net.feature_bytes]
                net.graph = True
                call(net, 1)
                put(f"{name} graph B=1", call(net, 1))
                sz.append(net.last_graph_nodes)
            sizes[name] = sz
        finally:
            _lib.check(lib.rgbm_debug_flags(0), "rgbm_debug_flags")

    for dt in ("bf16", "bf16x3", "fp32"):
        for opts in ({"sweep_f16": 0}, {"upconv": 0}, {"upconv": 3}, {"upconv": 4}, {"stem": 0}, {"fuse_final": 0}, {"igemm_conv6": 0},
                     {"sparse_dec": 1}, {"sparse_tail": 0}):
            if dt == "fp32" and next(iter(opts)) in ("sweep_f16", "igemm_conv6", "sparse_dec", "sparse_tail", "stem"):
                continue      # no pack of an fp32 net answers to these: the defaults above cover it
            config(f"{dt} options {opts}", dt, options=opts)
        for flag in (1024, 2048, 4096, 524288):
            config(f"{dt} debug flag {flag}", dt, flags=flag)
    config("fp16", "fp16")
    config("fp16 options {'sparse_dec': 0}", "fp16", options={"sparse_dec": 0})
    for rp in (True, False):
        config(f"bf16 baseline regress_pose={rp} options {{'upconv': 0, 'stem': 0}}", "bf16", state=synth.baseline_state_dict(seed=0, regress_pose=rp),
               arch="baseline", regress_pose=rp, options={"upconv": 0, "stem": 0})
        config(f"bf16 baseline regress_pose={rp} debug flags 1024 + 2048 + 524288", "bf16", flags=1024 | 2048 | 524288,
               state=synth.baseline_state_dict(seed=0, regress_pose=rp), arch="baseline", regress_pose=rp)
    for dt in ("bf16", "bf16x3"):
        net = AdaPoseNet(sd, dtype=dt, dropout=0.1, dropout_seed=3)
        i = inputs[2]
        put(f"{dt} forward_samples S=2 B=2", net.forward_samples(i["img1"], i["choose1"], i["img2"], i["choose2"], i["P1"], i["P2"], i["depths"], 2))
        sizes[f"{dt} samples_workspace_bytes"] = [net.samples_workspace_bytes(2, 2)]
    # what a captured forward consists of, and what the plan asks for
    for dt in ("bf16", "bf16x3", "fp32"):
        net = AdaPoseNet(sd, dtype=dt, graph=True)
        for rep in range(2):
            call(net, 1)
        sizes[f"{dt} last_graph_nodes"] = [net.last_graph_nodes]
        sizes[f"{dt} workspace_bytes"] = [net.workspace_bytes(B) for B in (1, 2, 3, 256)]
        sizes[f"{dt} feature_bytes"] = [net.feature_bytes]
    put("sizes", {k: np.asarray(v, np.int64) for k, v in sizes.items()})
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])

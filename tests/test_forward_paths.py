"""CPU-only: which kernel paths a forward runs is one pure decision (csrc/forward_paths.cpp, exported as rgbm_forward_paths).  It agrees
with the parent commit's inline conditions (tests/forward_paths_ref.py) over two full cross products of what those conditions read, keeps
the invariants that tie the plan to the launches, gives the documented default rows, and answers to the four debug flags it reads."""
import ctypes as C
import itertools

import numpy as np
import pytest

from rgbmanip_amd import _lib

from forward_paths_ref import BF16, BF16X3, F16, F32, FACTS, N_FACTS, N_PATHS, PATHS, paths as ref_paths

DTYPES = (F32, BF16, F16, BF16X3)
FI = {k: i for i, k in enumerate(FACTS)}
PI = {k: i for i, k in enumerate(PATHS)}


def lib_paths(facts):
    facts = np.ascontiguousarray(facts, np.int32)
    out = np.empty((len(facts), N_PATHS), np.int32)
    i32p = C.POINTER(C.c_int32)
    _lib.check(_lib.load().rgbm_forward_paths(facts.ctypes.data_as(i32p), len(facts), out.ctypes.data_as(i32p)), "rgbm_forward_paths")
    return out


def base_facts(arch, dtype, B=1):
    """A handle as create() / create_baseline() build it for this storage type, default options (include/rgbm.h), a plain call of B poses."""
    v5, packs = arch == 0, dtype != F32
    return dict(arch=arch, dtype=dtype, norm_mode=0, cost_impl=3, sparse_tail=1, sparse_dec=2, sweep_f16=1, igemm_conv6=1, fuse_final=1, upconv=7,
                stem=int(packs), view2_heads=1, pose_x3=1, flags=0, stem_w=int(packs), sweep_w=int(v5 and packs), sweep_w_f16=int(v5 and dtype == BF16),
                w11_x3=int(v5 and dtype == BF16X3), w11_taps=int(v5 and packs), tail_ready=int(packs), tail_f16_ready=int(dtype == BF16), pmlp_table=1,
                psp_shape_ok=1, pose_shape_ok=int(dtype == BF16), dense=0, V=2 * B, Vh=2 * B, n_pts=1024)


def product(axes):
    """[rows, N_FACTS]: base_facts(arch, dtype) of every row, overridden by every combination of `axes` (name -> values; "arch" and "dtype" first)."""
    names = list(axes)
    rows = []
    for arch, dtype in itertools.product(axes["arch"], axes["dtype"]):
        base = np.array([base_facts(arch, dtype)[k] for k in FACTS], np.int32)
        rest = [n for n in names if n not in ("arch", "dtype")]
        combos = np.array(list(itertools.product(*[axes[n] for n in rest])), np.int32)
        block = np.tile(base, (len(combos), 1))
        for j, n in enumerate(rest):
            if n == "flags":
                block[:, FI[n]] |= combos[:, j]
            else:
                block[:, FI[n]] = combos[:, j]
        rows.append(block)
    return np.concatenate(rows)


@pytest.fixture(scope="module")
def cost_group():
    # upconv bit 2 alone moves the cost paths (the f16 feature form needs the one-kernel up_3 + final); 3 | 4 = the default 7
    return product(dict(arch=(0, 1), dtype=DTYPES, norm_mode=(0, 1), cost_impl=(0, 1, 2, 3), sparse_tail=(0, 1), sparse_dec=(0, 1, 2), sweep_f16=(0, 1),
                        igemm_conv6=(0, 1), upconv=(3, 7), flags=(0, 4096), dense=(0, 1), sweep_w_f16=(0, 1), tail_f16_ready=(0, 1), w11_x3=(0, 1)))


@pytest.fixture(scope="module")
def front_group():
    g = product(dict(arch=(0, 1), dtype=DTYPES, stem=(0, 1), upconv=tuple(range(8)), fuse_final=(0, 1),
                     flags=tuple(a | b | c for a in (0, 1024) for b in (0, 2048) for c in (0, 524288)), V=(2, 32, 34), n_pts=(1024, 1000),
                     pmlp_table=(0, 1), psp_shape_ok=(0, 1), pose_shape_ok=(0, 1)))
    g[:, FI["Vh"]] = g[:, FI["V"]]
    return g


def test_agrees_with_the_parent_commits_conditions(cost_group, front_group):
    assert len(cost_group) == 2 * 4 * 2 * 4 * 2 * 3 * 2 * 2 * 2 * 2 * 2 * 8 and len(front_group) == 2 * 4 * 2 * 8 * 2 * 8 * 3 * 2 * 8
    for name, g in (("cost", cost_group), ("front / heads", front_group)):
        got, want = lib_paths(g), ref_paths(g)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (name, len(bad), dict(zip(FACTS, g[bad[0]])), dict(zip(PATHS, got[bad[0]])), dict(zip(PATHS, want[bad[0]])))


def test_invariants_tie_the_plan_to_the_launches(cost_group, front_group):
    for g in (cost_group, front_group):
        # create() uploads the f16 form of the sweep weights only next to the sweep pack itself (adapose.cpp: create_cost), and
        # create_baseline() neither: a handle with the one and without the other does not exist, and nothing is promised for it
        g = g[~((g[:, FI["sweep_w_f16"]] == 1) & (g[:, FI["sweep_w"]] == 0))]
        p = {k: lib_paths(g)[:, i] for k, i in PI.items()}
        x3 = g[:, FI["dtype"]] == BF16X3
        reads_vol = (p["cost_body"] == 1) | (p["cost_body"] == 2) | (p["conv0"] == 1)      # launch_build_volume in front of each of them
        assert np.array_equal(p["vol"] == 1, reads_vol)
        assert np.array_equal(p["bn_scratch"] == 1, p["cost_body"] == 1)
        assert np.all(p["tail_sparse"][p["mask_level"] > 0] == 1)
        assert np.array_equal(p["sweep_list"] == 1, p["mask_level"] == 2)
        assert np.all(g[:, FI["dense"]][p["tail_sparse"] == 1] == 0)
        f16 = p["feat_form"] == 2
        assert np.all(p["up3"][f16] == 2) and np.all(p["conv0"][f16] == 4) and np.array_equal(p["conv0"] == 4, f16 & (g[:, FI["arch"]] == 0))
        only = p["feat_form"] == 1
        # the split-pair map's readers are build_volume (bodies 1 / 2, conv0 1) and the halo tile with the fused warp (conv0 2)
        assert np.all(p["conv0"][only] == 5) and np.all(p["feat_copy"][only] == 0) and not np.any(reads_vol[only])
        assert np.array_equal(p["feat_copy"] == 1, x3 & ~only)


def test_documented_defaults():
    """One row per storage type: default options on a handle as create() builds it (include/rgbm.h's option table, README "Modes")."""
    rows = np.array([[base_facts(0, dt)[k] for k in FACTS] for dt in (BF16, BF16X3, F32, F16)], np.int32)
    bf16, x3, fp32, fp16 = (dict(zip(PATHS, r)) for r in lib_paths(rows))
    want = dict(stem=1, up3=2, feat_form=2, conv0=4, conv6_igemm=1, mask_level=2, tail_sparse=1, point_mlp=1, pose_mlp=1)
    assert {k: bf16[k] for k in want} == want
    assert (x3["feat_form"], x3["conv0"], x3["feat_copy"]) == (1, 5, 0)
    assert (fp32["conv0"], fp32["tail_sparse"], fp32["cost_body"], fp32["stem"]) == (2, 0, 3, 0)
    assert (fp16["conv0"], fp16["feat_form"], fp16["tail_sparse"]) == (3, 0, 1)


@pytest.mark.parametrize("flag,dtype,moved", [
    (1024, BF16, dict(psp_stage=(1, 2))),
    (2048, BF16, dict(point_mlp=(1, 0))),
    (524288, BF16, dict(pose_mlp=(1, 0))),
    # the halo-tile conv0 with the fused warp reads the storage type and every tile
    (4096, BF16, dict(conv0=(4, 2), feat_form=(2, 0), mask_level=(2, 0), sweep_list=(1, 0))),
    (4096, BF16X3, dict(conv0=(5, 2), feat_form=(1, 0), feat_copy=(0, 1), mask_level=(2, 0), sweep_list=(1, 0))),
    (4096, F32, {}),
])
def test_debug_flags_move_what_they_document(flag, dtype, moved):
    """include/rgbm.h, rgbm_debug_flags: 1024 / 2048 / 4096 / 524288, read from the process (facts[13] < 0) as a forward reads them."""
    lib = _lib.load()
    facts = base_facts(0, dtype)
    facts["flags"] = -1
    row = np.array([[facts[k] for k in FACTS]], np.int32)
    assert row.shape == (1, N_FACTS)
    try:
        _lib.check(lib.rgbm_debug_flags(0), "rgbm_debug_flags")
        before = dict(zip(PATHS, lib_paths(row)[0]))
        _lib.check(lib.rgbm_debug_flags(flag), "rgbm_debug_flags")
        after = dict(zip(PATHS, lib_paths(row)[0]))
    finally:
        lib.rgbm_debug_flags(0)
    assert {k: (before[k], after[k]) for k in PATHS if before[k] != after[k]} == moved

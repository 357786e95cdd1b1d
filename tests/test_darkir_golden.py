"""CPU checks of DarkIR's dilated-gate decoder block: the fp64 restatement (tests/darkir_ref.py) against the fixtures captured
from the reference (tools/capture_golden_darkir.py), the native module's state_dict against the reference's, the host-only plan
and sizing entry points, and the GPU parity case list against the plan forms."""
import ctypes as C
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import darkir_ref as D  # noqa: E402
from oracle.fixtures import check, load  # noqa: E402


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_darkir", os.path.join(ROOT, "tools", "capture_golden_darkir.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_reference_fixture(name):
    c, dil, extra, bhw, seed = G.CASES[name]
    gold = load(name)
    x, cot = G.case_io(c, bhw, seed)
    got = D.run(x, cot, D.make_state(D.dblock_shapes(c, len(dil), extra), seed), dil)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        check(k, v, gold, 1e-9, what=name + " ")
    # both halves are live: beta and gamma are non-zero, so every gradient is
    assert all(float(v.abs().max()) > 0 for v in got.values())


def test_bounds_table_is_the_host_error_of_the_restatement():
    """The committed bounds are what tools/darkir_bounds.py computes (two cheap cases recomputed here), one entry per case, dtype
    and tensor."""
    bounds = load("darkir_bounds")
    for name in ("sub_halo", "one_branch"):
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            errs, _ = D.host_errors(name, dtype)
            for k, v in errs.items():
                assert v / 3 <= float(bounds[f"{name}.{tag}.{k}"]) <= 3 * v, (name, tag, k)   # (summation order varies by host)
    for name, (shape, dil, extra) in D.PARITY_CASES.items():
        keys = ["y", "dx"] + ["g." + k for k in D.dblock_shapes(shape[1], len(dil), extra)]
        for tag in ("fp32", "bf16"):
            assert all(0 < float(bounds[f"{name}.{tag}.{k}"]) < 0.05 for k in keys), (name, tag)


def test_native_module_has_reference_keys_and_refuses_cpu(lib):
    from image_restoration_amd import darkir as N
    import image_restoration_amd
    assert image_restoration_amd.DBlock is N.DBlock
    keys = load("darkir_dblock_keys")
    for tag, args in (("dil149_extra", dict(c=32, dilations=[1, 4, 9], extra_depth_wise=True)),
                      ("dil1_plain", dict(c=16, dilations=[1], extra_depth_wise=False))):
        blk = N.DBlock(**args)
        sd = blk.state_dict()
        assert list(sd) == [str(k) for k in keys[tag + ".keys"]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys[tag + ".shapes"]]
        blk.load_state_dict(D.make_state(D.dblock_shapes(args["c"], len(args["dilations"]), args["extra_depth_wise"]), seed=5))
    with pytest.raises(RuntimeError, match="MI355X only"):
        blk(torch.zeros(1, 16, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        blk(torch.zeros(1, 16, 8, 8), adapter=None)
    assert N.LayerNorm2d(8).eps == 1e-6
    for bad in (dict(DW_Expand=1), dict(FFN_Expand=3)):
        with pytest.raises(NotImplementedError, match="DW_Expand = FFN_Expand = 2"):
            N.DBlock(16, **bad)
    for dil in ([0], [17], [1, 2, 3, 4, 5], []):
        with pytest.raises(NotImplementedError, match="1..16|1..4"):
            N.DBlock(16, dilations=dil)
    with pytest.raises(NotImplementedError, match="inside DBlock only"):
        N.Branch(16, 1, 4)(torch.zeros(1, 16, 8, 8))


# DarkIR's four decoder planes at bs 8 with dilations [1, 4, 9]: (c, H = W) -> the pinned plan
DECODER_PLANS = {
    (32, 256): dict(tile_rows=32, tile_cols=64, halo=9, lds_bytes=32800, grid_x=32, grid_y=32, grid_z=8, pool_partials=32,
                    z_stored=False, fwd_ws_bytes=32768, bwd_splits=16, bwd_ws_bytes=135200768),
    (64, 128): dict(tile_rows=32, tile_cols=64, halo=9, lds_bytes=32800, grid_x=8, grid_y=64, grid_z=8, pool_partials=8,
                    z_stored=False, fwd_ws_bytes=16384, bwd_splits=8, bwd_ws_bytes=68091904),
    (128, 64): dict(tile_rows=32, tile_cols=64, halo=9, lds_bytes=32800, grid_x=2, grid_y=128, grid_z=8, pool_partials=2,
                    z_stored=False, fwd_ws_bytes=8192, bwd_splits=2, bwd_ws_bytes=34045952),
    (256, 32): dict(tile_rows=32, tile_cols=32, halo=9, lds_bytes=20000, grid_x=1, grid_y=256, grid_z=8, pool_partials=1,
                    z_stored=False, fwd_ws_bytes=8192, bwd_splits=1, bwd_ws_bytes=17268736),
}


def test_dilgate_plan_pinned_values_errors_and_lds(lib):
    from image_restoration_amd import ops
    for (c, hw), want in DECODER_PLANS.items():
        assert ops.dilgate_plan(8, c, hw, hw, torch.bfloat16, (1, 4, 9)) == want, (c, hw)
    # the LDS tile is two planes of (32 + 2 halo) x (tile columns + 2 halo) floats
    p = ops.dilgate_plan(8, 32, 256, 256, torch.bfloat16, (1, 4, 9))
    assert p["lds_bytes"] == 2 * (32 + 18) * (64 + 18) * 4
    L, out = lib, (lib.c_i64 * 12)()

    def plan(n, dil, o=out):
        arr = (C.c_int * 8)(*dil)
        return L.lib().mi_dilgate_plan(2, 16, 20, 20, L.MI_F32, n, arr, o)

    assert plan(3, (1, 4, 9)) == 0
    for n, dil, msg in ((0, (1,), b"n_dil=0"), (5, (1, 1, 1, 1, 1), b"n_dil=5"), (2, (1, 0), b"dilation 0"), (2, (17, 1), b"dilation 17")):
        assert plan(n, dil) == -1
        assert msg in L.lib().mi_last_error()
    assert plan(1, (1,), None) == -1 and b"null" in L.lib().mi_last_error()
    assert L.lib().mi_dilgate_plan(2, 16, 20, 20, L.MI_F32, 1, None, out) == -1
    assert L.lib().mi_dilgate_plan(2, 16, 20, 20, 7, 1, (C.c_int * 1)(1), out) == -1 and b"bad dtype 7" in L.lib().mi_last_error()
    assert L.lib().mi_dilgate_plan(2, 0, 20, 20, L.MI_F32, 1, (C.c_int * 1)(1), out) == -1
    # within the CU's 160 KiB (and the 64 KiB a launch gets without raising the kernel's limit) for every plane and halo
    for H in (1, 5, 31, 32, 33, 64, 257):
        for W in (1, 7, 32, 33, 64, 65, 1000):
            for d in range(1, 17):
                q = ops.dilgate_plan(1, 1, H, W, torch.float32, (d,))
                assert q["halo"] == d and q["tile_cols"] == (64 if W > 32 else 32)
                assert q["lds_bytes"] == 2 * (32 + 2 * d) * (q["tile_cols"] + 2 * d) * 4 <= 64 * 1024
                assert q["pool_partials"] == q["grid_x"] == -(-H // 32) * -(-W // q["tile_cols"])
                assert q["bwd_splits"] == min(q["grid_x"], 16)


def test_dblock_sizing_without_gpu(lib):
    from image_restoration_amd import ops
    for dtype in (torch.float32, torch.bfloat16):
        saved, ws = ops.dblock_sizes(2, 32, 20, 24, dtype, (1, 4, 9), True)
        es = 4 if dtype == torch.float32 else 2
        # x0, g, y, y0, h (c planes) and x1, x2, u (2c planes): eleven c-plane sets
        assert saved >= 11 * 2 * 32 * 480 * es and ws > 0
        plain, _ = ops.dblock_sizes(2, 32, 20, 24, dtype, (1,), False)
        assert 0 < plain < saved                    # no extra_conv: its input and output are one tensor
    assert ops.dblock_sizes(1, 256, 8, 8, torch.bfloat16, (16, 16, 2, 1), True)[0] > 0
    for bad in (dict(Cc=257), dict(Cc=0), dict(B=0), dict(H=0), dict(dilations=(1, 17)), dict(dilations=()), dict(dilations=(1, 2, 3, 4, 5))):
        args = dict(B=2, Cc=32, H=20, W=24, dtype=torch.float32, dilations=(1, 4, 9), extra=True)
        args.update(bad)
        assert ops.dblock_sizes(**args) == (0, 0), bad
        assert lib.lib().mi_last_error()
    assert lib.lib().mi_dblock_saved_bytes(None) == 0
    assert lib.lib().mi_dilgate_bwd_workspace(2, 16, 20, 20, 3, lib.MI_BF16) > 2 * 32 * 400 * 4   # dz, fp32
    assert lib.lib().mi_dilgate_bwd_workspace(2, 16, 20, 20, 5, lib.MI_BF16) == 0
    assert lib.lib().mi_dilgate_fwd_workspace(2, 16, 20, 20) > 0 and lib.lib().mi_dilgate_fwd_workspace(2, 16, 0, 20) == 0
    assert lib.lib().mi_pairconv3x3_bwd_workspace(2, 16, 20, 20) > 0 and lib.lib().mi_pairconv3x3_bwd_workspace(0, 16, 20, 20) == 0
    # null pointers are refused with an error code, not a crash
    assert lib.lib().mi_ln_fwd_eps(None, None, None, None, None, None, 1, 4, 16, 1, 1e-6, 0, None) == -1
    assert lib.lib().mi_pairconv3x3_fwd(None, None, None, None, 1, 4, 8, 8, 0, None) == -1
    s = ops._dblock_shape(2, 32, 20, 24, lib.MI_F32, (1, 4, 9), True)
    assert lib.lib().mi_dblock_fwd(C.byref(s), None, None, None, None, None, None) == -1


def test_parity_cases_reach_every_plan_form(lib):
    """The GPU parity case list reaches every form mi_dilgate_plan can return: both tile widths, one tile and several, fewer
    weight-gradient workgroups than the cap and the cap of 16; z is never stored."""
    from image_restoration_amd import ops
    seen = set()
    for (B, c, H, W), dil, _ in D.PARITY_CASES.values():
        p = ops.dilgate_plan(B, c, H, W, torch.float32, dil)
        assert not p["z_stored"]
        seen.add((p["tile_cols"], min(p["grid_x"], 2), p["bwd_splits"] == 16))
    # (a 32-wide tile never reaches the cap inside a test's budget: 16 tiles of 32 rows are a 512-row plane of one column)
    assert seen == {(32, 1, False), (32, 2, False), (64, 2, False), (64, 2, True)}, seen
    halos = {max(dil) for _, dil, _ in D.PARITY_CASES.values()}
    assert {1, 9, 16} <= halos

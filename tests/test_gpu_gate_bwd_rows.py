"""The recomputing GDFN gate backward (dws_gate_bwd_rc_kernel, csrc/dwstream.hip) at every way its row loop can end.

The kernel walks a band three rows per loop trip (its 3-row windows are named by row mod 3, nothing is rotated) and finishes
with one or two single rows, so what matters is the band's row count mod 3, bands shorter than one trip, and waves whose lane
groups sit in bands of different heights (the ragged last band beside full ones).  Every case goes through the runner, the fp64
autograd reference, the NaN guard bands and the tolerances of test_gpu_dwconv.py, with random data, and asserts the plan it
means to reach.  The tall bands need >= 8192 waves, hence the large batches; with h <= 5 every channel is checked.

A deliberate economy: the 40 band-16 shapes (h, H, W) each run ONE of the four (entry, dtype) combinations, on a rotation that
gives every width and every height each combination (test_tables_reach_their_plans holds it to that); the full cross would be
160 cases of 2-4 s, most of it the fp64 reference on ~40 M elements.  The short planes and the band-32 / band-64 shapes run all
four.  A fault that needs one combination at one particular (H, W) of band 16 can therefore slip through."""
import math

import pytest
import torch

from test_gpu_dwconv import BF16, DEV, DTS, F32, Guarded, Mem, _guard_for, _ok, _p, lib, ops, plan, run

COMBOS = (("rc", "bf16"), ("rc_nob", "f32"), ("rc_nob", "bf16"), ("rc", "f32"))
WIDTHS = (16, 32, 64, 128, 256)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def _expect(pl, band, W, nb):
    G = 256 // W
    assert pl["family"] == "stream" and pl["band"] == band and pl["lpr"] == W // 4 and pl["nb"] == nb, pl
    assert pl["uni"] == (G == 1 or nb % G == 0), pl


def _batch_for_band16(h, H, W):
    """The smallest batch whose B * h planes reach 8192 waves with bands of 16 rows (and stay below that with 32)."""
    G = 256 // W
    return -(-8192 * G // (math.ceil(H / 16) * h))


# --------------------------------------------------------------------------- planes no taller than one loop trip (and a bit)
SHORT = [pytest.param(H, W, e, d, id=f"H{H}-W{W}-{e}-{d}")
         for H in (1, 2, 3, 4, 5, 7) for W in (256, 16) for e in ("rc", "rc_nob") for d in ("bf16", "f32")]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,entry,dt", SHORT)
def test_planes_shorter_than_the_row_loop(H, W, entry, dt):
    B, h = 2, 3
    _expect(plan(B, 2 * h, H, W, 3, entry), 8, W, 1)
    run(entry, DTS[dt], B, 2 * h, H, W, 3, rand=True, mem=Guarded(_guard_for(B, 2 * h, H, W, 3)), seed=H + W)


# --------------------------------------------------------------------------- ragged last bands at band 16, every row width
# (entry, dtype) walks the four combinations so that every width and every height meets each of them
RAGGED16 = [pytest.param(h, H, W, *COMBOS[(iH + iW + 2 * ih) % 4], id=f"h{h}-H{H}-W{W}-" + "-".join(COMBOS[(iH + iW + 2 * ih) % 4]))
            for ih, h in enumerate((5, 4)) for iH, H in enumerate((17, 31, 33, 50)) for iW, W in enumerate(WIDTHS)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,H,W,entry,dt", RAGGED16)
def test_ragged_last_band_of_16_rows(h, H, W, entry, dt):
    B = _batch_for_band16(h, H, W)
    _expect(plan(B, 2 * h, H, W, 3, entry), 16, W, math.ceil(H / 16))
    run(entry, DTS[dt], B, 2 * h, H, W, 3, rand=True, mem=Guarded(_guard_for(B, 2 * h, H, W, 3)), seed=H + W + h)


# --------------------------------------------------------------------------- one ragged case each at bands of 32 and 64 rows
TALL = [pytest.param(B, band, nb, e, d, id=f"B{B}-band{band}-{e}-{d}")
        for B, band, nb in ((8, 32, 2), (16, 64, 1)) for e, d in COMBOS]


@pytest.mark.gpu
@pytest.mark.parametrize("B,band,nb,entry,dt", TALL)
def test_ragged_last_band_of_32_and_64_rows(B, band, nb, entry, dt):
    """H = 40 at W = 256: bands of 32 + 8 rows, and one band of 64 that holds 40."""
    h, H, W = 512, 40, 256
    _expect(plan(B, 2 * h, H, W, 3, entry), band, W, nb)
    run(entry, DTS[dt], B, 2 * h, H, W, 3, rand=True, mem=Guarded(_guard_for(B, 2 * h, H, W, 3)), seed=band)


# --------------------------------------------------------------------------- accumulation into prefilled gradients
@pytest.mark.gpu
def test_accumulate_adds_to_prefilled_gradients_on_a_ragged_band():
    h, H, W = 5, 33, 64
    B = _batch_for_band16(h, H, W)
    _expect(plan(B, 2 * h, H, W, 3, "rc"), 16, W, 3)
    g = torch.Generator(device=DEV)
    g.manual_seed(91)
    pre = (torch.randint(-16, 17, (2 * h, 9), generator=g, device=DEV).float() / 2,
           torch.randint(-16, 17, (2 * h,), generator=g, device=DEV).float() / 2)
    run("rc", F32, B, 2 * h, H, W, 3, rand=True, mem=Mem(), seed=11, acc_prefill=pre)


# --------------------------------------------------------------------------- the two instantiations agree; calls repeat bitwise
def _call(dtype, B, h, H, W, want_dw, seed=21):
    """One mi_dwconv_gate_bwd_recompute call on random data: (dx, dW, db), the last two None without the weight gradient."""
    L, o = lib(), ops()
    C = 2 * h
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn((B, C, H, W), generator=g, device=DEV).to(dtype)
    dg = torch.randn((B, h, H, W), generator=g, device=DEV).to(dtype)
    w = torch.randn((C, 9), generator=g, device=DEV) / 3
    bias = 0.1 * torch.randn((C,), generator=g, device=DEV)
    dx = torch.empty_like(x)
    dw = torch.full((C, 9), float("nan"), device=DEV) if want_dw else None
    db = torch.full((C,), float("nan"), device=DEV) if want_dw else None
    ws = torch.empty(max(L.mi_dwconv_bwd_workspace(B, C, H, W, 3), 1), dtype=torch.uint8, device=DEV)
    _ok(L.mi_dwconv_gate_bwd_recompute(_p(dg), _p(x), _p(w), _p(bias), _p(dx), _p(dw), _p(db), B, C, H, W, 3, 0,
                                       0 if dtype == F32 else 1, _p(ws), o._stream()), "rc")
    torch.cuda.synchronize()
    return dx, dw, db


PAIR_SHAPES = [pytest.param(2, 3, 7, 256, 8, id="band8-H7-W256"),
               pytest.param(_batch_for_band16(5, 33, 64), 5, 33, 64, 16, id="band16-H33-W64")]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,h,H,W,band", PAIR_SHAPES)
def test_dx_without_the_weight_gradient_and_repeat_calls_are_bitwise(B, h, H, W, band, dtype):
    """The instantiation without the weight gradient (dW, db null) gives bitwise the dx of the one with it, and the same call
    twice gives bitwise equal dx, dW and db."""
    _expect(plan(B, 2 * h, H, W, 3, "rc"), band, W, math.ceil(H / band))
    dx, dw, db = _call(dtype, B, h, H, W, True)
    assert not (dx.float().isnan().any() or dw.isnan().any() or db.isnan().any())
    dx0, _, _ = _call(dtype, B, h, H, W, False)
    assert torch.equal(dx.view(torch.uint8), dx0.view(torch.uint8)), "dx differs when dW, db are not asked for"
    dx2, dw2, db2 = _call(dtype, B, h, H, W, True)
    assert torch.equal(dx.view(torch.uint8), dx2.view(torch.uint8)), "dx differs between two identical calls"
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "dW / db differ between two identical calls"


# --------------------------------------------------------------------------- the tables reach what they name (no GPU needed)
def test_tables_reach_their_plans():
    seen = set()
    for h in (5, 4):
        for H in (17, 31, 33, 50):
            for W in WIDTHS:
                pl = ops().dwconv_plan(_batch_for_band16(h, H, W), 2 * h, H, W, 3, "gate_bwd")
                _expect(pl, 16, W, math.ceil(H / 16))
                seen.add((W, pl["uni"], (H - 16 * (pl["nb"] - 1)) % 3))
    for W in WIDTHS:
        assert {s[2] for s in seen if s[0] == W} == {0, 1, 2}, f"W={W}: a last band's rows mod 3 is missing"
    assert any(not s[1] for s in seen) and any(s[1] for s in seen)
    for W in WIDTHS:
        assert {c.values[3:] for c in RAGGED16 if c.values[2] == W} == set(COMBOS), f"W={W}: an entry / dtype is missing"

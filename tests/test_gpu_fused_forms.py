"""Every instance of the fused half-block forwards (csrc/fused_gdfn.hip, csrc/fused_mdta.hip) against the fp64 oracle and against
the unfused chain, on shapes that hold every seam: at least two tile rows and two tile columns (an interior corner halo pixel
and all four image borders), two images (the image stride), a ragged and an exact last chunk of the hidden dimension, both
LayerNorm kinds, bias on and off.  The case tables, the assertions and the reasoning behind the parameters are in
tests/fused_forms.py; tests/test_cabi.py checks without a GPU that the tables reach every instance the dispatch lists hold and
that the assertions see five injected faults.

Every case first asserts from ops.gdfn_fused_plan / ops.mdta_fused_plan (the same plan the launcher follows) that the call
reaches the instance the row is written for.  Packs are built and run under the same switches (a pack built for one chunk
width and run under another gives wrong numbers without an error: INTEGRATION.md)."""
import functools
import math

import pytest
import torch

import fused_forms as FF
from fused_forms import rel
from test_gpu_fused import _oracle_attn_half

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _ops():
    from image_restoration_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _gdfn_reference(C, pset, shape):
    """(y, state, kind, hidden, fp64 oracle) of a case: computed once, shared by the cases that use it, never written to."""
    sd, kind, hidden = FF.gdfn_state(C, pset)
    y = FF.gdfn_input(shape)
    return y, sd, kind, hidden, FF._oracle_half_block(y, sd, kind)


def _device_params(sd, kind):
    ln_w = sd["norm2.body.weight"].to(DEV).float()
    ln_b = sd["norm2.body.bias"].to(DEV).float() if kind == "WithBias" else None
    return ln_w, ln_b, FF._ffn_params(sd, DEV)


def _chain(ops, yb, ln_w, ln_b, kind, params):
    yn, mean, rstd = ops.ln_fwd(yb, ln_w, ln_b, kind == "WithBias", want_stats=True)
    return ops.gdfn_fwd(yn, yb, params, False)[0], yn, mean, rstd


def _f8_scales(ops, yn, ln_w, params, C):
    """As restormer.fp8_calibrate derives them, for the fused kernel's operands (tests/test_gpu_f8.py)."""
    from image_restoration_amd.restormer import _f8_pow2
    g = ops.dwconv_gate_fwd(ops.conv1x1(yn, params[0], params[1]), params[2], params[3], want_y=False)[1]
    wfold = float((params[0].reshape(params[0].shape[0], -1) * ln_w[None, :]).abs().max())
    return (_f8_pow2(math.sqrt(C)), _f8_pow2(wfold), _f8_pow2(4 * float(g.abs().max())), _f8_pow2(float(params[4].abs().max())))


@pytest.mark.parametrize("case", FF.GDFN_CASES, ids=FF.case_id)
def test_gdfn_fused_instance_vs_oracle_and_chain(case, monkeypatch):
    """One instance of the fused GDFN forward: the three bars of tests/test_gpu_fused.py (out 2e-2, branch 4e-2, no further from
    the oracle than 1.5 e_chain + 4e-3), the statistics against ln_fwd (1e-5) where the entry emits them, a bit-identical second
    call; SAVE: h0 and g against the chain's blob (1.2e-2, 2e-2) and h0 against the oracle's project_in(LN(y)); F8: the bars of
    tests/test_gpu_f8.py against the bf16 launch under the same switches (which the same call holds to the oracle)."""
    ops = _ops()
    inst, entry, cfg, shape, pset = case
    y, sd, kind, hidden, ref = _gdfn_reference(shape[1], pset, shape)
    wb = kind == "WithBias"
    FF.set_switches(monkeypatch, cfg)
    plan = FF.reach(ops, inst, entry, shape, hidden)
    assert plan["tiles_y"] >= 2 or shape[2] == 8
    yb = y.to(DEV).to(BF16)
    ln_w, ln_b, params = _device_params(sd, kind)
    assert ops.gdfn_fused_ok(yb, hidden)
    pack = ops.gdfn_fused_pack(yb, ln_w, ln_b, params)
    assert pack.numel() == plan["pack_bytes"]
    FF.assert_pack_padding(pack, shape[1], hidden, plan["pack_pc"], params[4])
    chain, yn, mean_c, rstd_c = _chain(ops, yb, ln_w, ln_b, kind, params)
    what = FF.case_id(case)
    if entry == "train":
        assert ops.gdfn_fused_train_ok(yb, hidden)
        out, saved, mean, rstd = ops.gdfn_fused_fwd_train(yb, pack, hidden, wb)
        out2, saved2, _, _ = ops.gdfn_fused_fwd_train(yb, pack, hidden, wb)
        chain_t, saved_c, _, _ = ops.gdfn_fwd(yb, yb, params, True, ln=(ln_w, ln_b, True))
        torch.cuda.synchronize()
        assert torch.equal(saved, saved2) and saved.numel() == saved_c.numel()
        h0, g = FF.split_saved(saved, shape, hidden)
        h0_c, g_c = FF.split_saved(saved_c, shape, hidden)
        FF.assert_saved(h0, g, h0_c, g_c, FF.oracle_h0(y, sd, kind), what)
        assert rel(chain_t, ref) < FF.BAR_OUT
    elif entry == "f8":
        out, mean, rstd = ops.gdfn_fused_fwd(yb, pack, hidden, wb, want_stats=True)      # the bf16 launch of the same pack
        out2 = ops.gdfn_fused_fwd(yb, pack, hidden, wb)[0]
        scales = _f8_scales(ops, yn, ln_w, params, shape[1])
        got = ops.gdfn_fused_fwd(yb, pack, hidden, wb, f8=scales)[0]
        got2 = ops.gdfn_fused_fwd(yb, pack, hidden, wb, f8=scales)[0]
        torch.cuda.synchronize()
        assert torch.isfinite(got.float()).all() and torch.equal(got, got2)
        branch = out.float() - yb.float()
        err = float((got.float() - out.float()).abs().max() / branch.abs().max())
        rms = float((got.float() - out.float()).pow(2).mean().sqrt() / branch.pow(2).mean().sqrt())
        print(f"{what}: fp8 vs bf16 launch: worst {err:.3e} rms {rms:.3e}")
        assert 0 < err < FF.BAR_F8_MAX and rms < FF.BAR_F8_RMS, (err, rms)
    else:
        out, mean, rstd = ops.gdfn_fused_fwd(yb, pack, hidden, wb, want_stats=True)
        out2 = ops.gdfn_fused_fwd(yb, pack, hidden, wb)[0]
    torch.cuda.synchronize()
    FF.assert_half_block(out, chain, y, ref, what)
    assert rel(mean, mean_c) < FF.BAR_STATS and rel(rstd, rstd_c) < FF.BAR_STATS
    assert torch.equal(out, out2), "a second call gave another result"


@pytest.mark.parametrize("inst,shape,pset", FF.XCD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_gdfn_xcd_tile_relabelling_changes_nothing(inst, shape, pset, monkeypatch):
    """tiles % 16 == 0 on 32-wide tiles: the workgroups are relabelled so that vertical neighbours share an XCD.  A pure
    relabelling of tiles: the plan shows it on by default and off under MI_FG_NOXCD=1, the outputs are bit-identical, and both
    meet the oracle bars."""
    ops = _ops()
    entry = "train" if inst[6] else "inference"
    y, sd, kind, hidden, ref = _gdfn_reference(shape[1], pset, shape)
    wb = kind == "WithBias"
    yb = y.to(DEV).to(BF16)
    ln_w, ln_b, params = _device_params(sd, kind)
    got = {}
    for noxcd in (False, True):
        FF.set_switches(monkeypatch, "", noxcd=noxcd)
        plan = FF.reach(ops, inst, entry, shape, hidden)
        assert plan["xcd_pairs"] == (not noxcd) and plan["grid"] % 16 == 0 and plan["tw"] == 32
        pack = ops.gdfn_fused_pack(yb, ln_w, ln_b, params)
        if entry == "train":
            out, saved, _, _ = ops.gdfn_fused_fwd_train(yb, pack, hidden, wb)
            got[noxcd] = (out, saved)
        else:
            got[noxcd] = ops.gdfn_fused_fwd(yb, pack, hidden, wb, want_stats=True)
    torch.cuda.synchronize()
    for a, b in zip(got[False], got[True]):
        assert torch.equal(a, b)
    chain = _chain(ops, yb, ln_w, ln_b, kind, params)[0]
    FF.assert_half_block(got[False][0], chain, y, ref, f"xcd_pairs {shape}")


def test_gdfn_fourth_form_uneven_persistent_ranges(monkeypatch):
    """fg4's persistent tile ranges where 256 / B caps the workgroups per image (S = 4) and the 10 tiles do not divide by it
    (ranges of 3, 3, 2, 2 tiles): a batch of 52 copies of two distinct images; the two are held to the oracle, and every copy
    equals its original bit for bit."""
    ops = _ops()
    inst, cfg, shape, pset, S, tiles = FF.FG4_RANGES
    two = (2,) + shape[1:]
    y, sd, kind, hidden, ref = _gdfn_reference(shape[1], pset, two)
    wb = kind == "WithBias"
    FF.set_switches(monkeypatch, cfg)
    plan = FF.reach(ops, inst, "inference", shape, hidden)
    assert plan["S"] == S == 256 // shape[0] and plan["tiles_x"] * plan["tiles_y"] == tiles and tiles % S != 0
    idx = torch.arange(shape[0]) % 2
    yb = y[idx].to(DEV).to(BF16)
    ln_w, ln_b, params = _device_params(sd, kind)
    out, mean, rstd = ops.gdfn_fused_fwd(yb, ops.gdfn_fused_pack(yb, ln_w, ln_b, params), hidden, wb, want_stats=True)
    chain, _, mean_c, rstd_c = _chain(ops, yb[:2], ln_w, ln_b, kind, params)
    torch.cuda.synchronize()
    FF.assert_half_block(out[:2], chain, y, ref, "fg4 uneven ranges")
    assert rel(mean[:2], mean_c) < FF.BAR_STATS and rel(rstd[:2], rstd_c) < FF.BAR_STATS
    for i in range(2, shape[0]):
        assert torch.equal(out[i], out[i % 2]) and torch.equal(mean[i], mean[i % 2]) and torch.equal(rstd[i], rstd[i % 2]), i


@pytest.mark.parametrize("entry,cfg,shape,hidden", FF.GDFN_REFUSALS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gdfn_entry_without_an_instance_is_refused_cleanly(entry, cfg, shape, hidden, monkeypatch):
    """A switch string that leaves an entry without a kernel: the plan (and the _ok predicate where the entry has one) says so
    beforehand, the launcher raises, and nothing is written - out, statistics and blob keep their fill."""
    ops = _ops()
    from image_restoration_amd import _lib as L
    import ctypes as C
    FF.set_switches(monkeypatch, cfg)
    assert not ops.gdfn_fused_plan(shape, hidden, entry)["covered"]
    assert ops.gdfn_fused_plan(shape, hidden, "inference")["covered"]          # the pack exists: only this entry has no kernel
    yb = FF.gdfn_input(shape).to(DEV).to(BF16)
    sd, kind, _ = FF.gdfn_state(shape[1], "rw")
    ln_w, ln_b, params = _device_params(sd, kind)
    pack = ops.gdfn_fused_pack(yb, ln_w, ln_b, params)
    s = L.GdfnFusedShape(shape[0], shape[1], hidden, shape[2], shape[3], 1)
    out = torch.full_like(yb, 7.0)
    mean = torch.full((shape[0], shape[2] * shape[3]), 7.0, device=DEV)
    rstd = mean.clone()
    p = f = lambda t: t.data_ptr()
    if entry == "train":
        assert not ops.gdfn_fused_train_ok(yb, hidden)
        saved = torch.full((L.lib().mi_gdfn_saved_bytes(C.byref(L.GdfnShape(shape[0], shape[1], hidden, shape[2], shape[3], L.MI_BF16, 3, 0))),),
                           7, dtype=torch.uint8, device=DEV)
        rc = L.lib().mi_gdfn_fused_fwd_train(C.byref(s), p(pack), p(yb), p(out), f(mean), f(rstd), p(saved), None)
        assert bool((saved == 7).all())
        with pytest.raises(RuntimeError, match="gdfn_fused_fwd_train"):
            ops.gdfn_fused_fwd_train(yb, pack, hidden, True)
    else:
        sc = L.F8Scales(1.0, 1.0, 1.0, 1.0)
        rc = L.lib().mi_gdfn_fused_fwd_f8(C.byref(s), p(pack), C.byref(sc), p(yb), p(out), None)
        with pytest.raises(RuntimeError, match="gdfn_fused_fwd_f8"):
            ops.gdfn_fused_fwd(yb, pack, hidden, True, f8=(1.0, 1.0, 1.0, 1.0))
    torch.cuda.synchronize()
    assert rc == -1
    assert bool((out == 7).all()) and bool((mean == 7).all()) and bool((rstd == 7).all())


def test_gdfn_inference_refuses_uncovered_shapes_cleanly():
    ops = _ops()
    from image_restoration_amd import _lib as L
    import ctypes as C
    for shape, hidden in (((1, 192, 16, 64), 510), ((1, 48, 16, 32), 127), ((1, 96, 12, 64), 255)):
        assert not ops.gdfn_fused_plan(shape, hidden, "inference")["covered"]
        yb = torch.zeros(shape, dtype=BF16, device=DEV)
        assert not ops.gdfn_fused_ok(yb, hidden)
        out, pack = torch.full_like(yb, 7.0), torch.zeros(4096, dtype=torch.uint8, device=DEV)
        s = L.GdfnFusedShape(shape[0], shape[1], hidden, shape[2], shape[3], 1)
        assert L.lib().mi_gdfn_fused_fwd(C.byref(s), pack.data_ptr(), yb.data_ptr(), out.data_ptr(),
                                         None, None, None) == -1
        torch.cuda.synchronize()
        assert bool((out == 7).all())


# ------------------------------------------------------------------------------------------------ fused MDTA, pass A
@pytest.mark.parametrize("case", FF.MDTA_CASES, ids=FF.mdta_case_id)
def test_mdta_fused_form_vs_oracle_and_chain(case, monkeypatch):
    """Both forms of pass A for every kind that has them, on even and uneven persistent tile ranges: the bars of
    test_mdta_fused_pass_a_vs_oracle_and_chain (out 2e-2, no further from the oracle than 1.5 e_chain + 4e-3, statistics 1e-5 /
    1e-4, bit-reproducible)."""
    ops = _ops()
    from oracle import restormer_ref as R
    from oracle.fixtures import seeded_input
    kind, c, heads, cfg, form, shape, bias, ln_kind, (tiles, S) = case
    FF.set_switches(monkeypatch, fm_cfg=cfg)
    plan = ops.mdta_fused_plan(shape, heads)
    assert (plan["covered"], plan["kind"], plan["form"]) == (True, kind, form), plan
    assert (plan["tiles_x"] * plan["tiles_y"], plan["S"], plan["grid"]) == (tiles, S, shape[0] * S), plan
    assert plan["part_mult"] == (8 if form == "fourth" else 1)
    sd = R.make_block_state(c, heads, 2.66, bias, ln_kind, seed=230 + c + heads)
    x = seeded_input(shape, 2300 + c).to(DEV).to(BF16)
    ref = _oracle_attn_half(x.float().cpu(), sd, heads, ln_kind)
    ln = (sd["norm1.body.weight"].to(DEV), sd["norm1.body.bias"].to(DEV) if "norm1.body.bias" in sd else None)
    keys = ["attn.temperature", "attn.qkv.weight", "attn.qkv.bias", "attn.qkv_dwconv.weight", "attn.qkv_dwconv.bias",
            "attn.project_out.weight", "attn.project_out.bias"]
    att = tuple(sd[k].to(DEV).float().contiguous() if k in sd else None for k in keys)
    assert ops.mdta_fused_ok(x, heads, 3)
    pack = ops.mdta_fused_pack(x, heads, ln[0], ln[1], att)
    assert pack.numel() == plan["pack_bytes"]
    wb = ln_kind == "WithBias"
    y, mean, rstd = ops.mdta_fused_fwd(x, pack, att, heads, wb, x, want_stats=True)
    xn, mean_r, rstd_r = ops.ln_fwd(x, ln[0], ln[1], wb, want_stats=True)
    chain, _ = ops.mdta_fwd(xn, x, att, heads, False)
    e_or, e_ch = rel(y, ref), rel(chain, ref)
    print(f"{FF.mdta_case_id(case)}: out {e_or:.3e} chain {e_ch:.3e}")
    assert e_or < 2e-2, (e_or, e_ch)
    assert e_or < 1.5 * e_ch + 4e-3, (e_or, e_ch)
    assert rel(mean, mean_r) < 1e-5 and rel(rstd, rstd_r) < 1e-4
    y2, _, _ = ops.mdta_fused_fwd(x, pack, att, heads, wb, x)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("shape,heads", FF.MDTA_REFUSALS)
def test_mdta_uncovered_shape_is_refused_cleanly(shape, heads):
    ops = _ops()
    from image_restoration_amd import _lib as L
    import ctypes as C
    assert not ops.mdta_fused_plan(shape, heads)["covered"]
    x = torch.zeros(shape, dtype=BF16, device=DEV)
    assert not ops.mdta_fused_ok(x, heads) and not ops.mdta_fused_pays(x, heads)
    out, blob = torch.full_like(x, 7.0), torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    c = shape[1]
    t, w = torch.ones(heads, device=DEV), torch.zeros((c, c), device=DEV)
    s = L.MdtaShape(shape[0], c, heads, shape[2], shape[3], L.MI_BF16, 3)
    p = f = lambda v: v.data_ptr()
    pp = L.MdtaParams(f(t), None, None, None, None, f(w), None)
    assert L.lib().mi_mdta_fused_fwd(C.byref(s), C.byref(pp), p(blob), 1, p(x), p(x), p(out), None, None, p(blob), None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all())

"""Case tables, inputs, assertions and a CPU model of the fused half-block forwards (csrc/fused_gdfn.hip, csrc/fused_mdta.hip).

Shared by tests/test_gpu_fused_forms.py (which runs the kernels) and tests/test_cabi.py (which, without a GPU, checks that the
tables reach every instance the dispatch lists can select, that the assertions pass on correct bf16 arithmetic and that they
fail on five injected faults).  A plain module: no fixtures, no pytest settings.

An INSTANCE is what ops.gdfn_fused_plan reports: ("tile", C, TH, TW, PC, NW, SAVE, F8) for fg_fwd_kernel<C,TH,TW,PC,NW,F8,SAVE>
and ("fourth", C, SAVE) for fg4_fwd_kernel<C,2,SAVE>.  Every row of a table names the instance it must reach, the MI_FG_CFG
string that selects it, and the shape; reach() asserts from the plan that the call gets there, so a switch string the
selection quietly ignores (pc32 with 16-row tiles, say) fails instead of testing the default twice."""
import os
import re

import torch

from oracle import restormer_ref as R
from oracle.fixtures import seeded_input
from test_gpu_fused import _ffn_params, _oracle_half_block, rel      # the suite's helpers, not copies of them

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------- the bars (tests/test_gpu_fused.py)
BAR_OUT, BAR_BRANCH = 2e-2, 4e-2           # out and the branch out - y against the fp64 oracle, of the tensor's largest magnitude
CHAIN_FACTOR, CHAIN_SLACK = 1.5, 4e-3      # no further from the oracle than 1.5 e_chain + 4e-3
BAR_STATS = 1e-5                           # LayerNorm statistics against ln_fwd
BAR_H0, BAR_G = 1.2e-2, 2e-2               # the saved blob against the chain's (and h0 against the oracle's project_in(LN(y)))
BAR_F8_MAX, BAR_F8_RMS = 0.12, 0.1         # fp8 operands against the bf16 launch: worst element / rms, of the branch (tests/test_gpu_f8.py)

# ---------------------------------------------------------------------------------------------- parameters
# hidden widths: at C = 48, 127 (last chunk holds 15 of 16 or 31 of 32 pairs) and 96 (exact chunks, ffn factor 2.0); at C = 96,
# 255 and 192.  Four parameter sets per width pair, so that both LayerNorm kinds meet bias on and off and the folded project_in
# bias b' = b_in + W_in beta is never zero (a zero b' cannot show the padding fault).  BIAS_SCALE multiplies the oracle's 0.1 N
# conv biases and BETA the LayerNorm beta: with the stock 0.1 N / 0.2 N a b' leaking into the zero padding moves the branch by
# 5 - 7 % only, under 3 x its 4 % bar; test_cabi's fault check holds these values to that cap.
BIAS_SCALE, BETA, GAMMA = 4.0, 0.8, 0.3
FFN = {(48, "ragged"): 2.66, (48, "exact"): 2.0, (96, "ragged"): 2.66, (96, "exact"): 2.0}
HIDDEN = {(48, "ragged"): 127, (48, "exact"): 96, (96, "ragged"): 255, (96, "exact"): 192}
PARAMS = {                                  # name -> (chunk, conv bias, LayerNorm kind)
    "rb": ("ragged", True, "BiasFree"), "ew": ("exact", False, "WithBias"),
    "rw": ("ragged", False, "WithBias"), "eb": ("exact", True, "BiasFree"),
    "rB": ("ragged", True, "WithBias"),
}


def gdfn_state(C, pset):
    """Seeded block parameters for a parameter set, with a non-trivial LayerNorm affine (so that its fold into project_in is
    exercised) and biases large enough for the padding fault (see BIAS_SCALE)."""
    chunk, bias, kind = PARAMS[pset]
    sd = R.make_block_state(C, 1, FFN[(C, chunk)], bias, kind, seed=400 + C + sum(map(ord, pset)))
    g = torch.Generator().manual_seed(5 + C)
    sd["norm2.body.weight"] = 1.0 + GAMMA * torch.randn(C, generator=g)
    if kind == "WithBias":
        sd["norm2.body.bias"] = BETA * torch.randn(C, generator=g)
    if bias:
        for k in ("ffn.project_in.bias", "ffn.dwconv.bias", "ffn.project_out.bias"):
            sd[k] = sd[k] * BIAS_SCALE
    assert sd["ffn.project_out.weight"].shape[1] == HIDDEN[(C, chunk)]
    return sd, kind, HIDDEN[(C, chunk)]


def gdfn_input(shape, seed=0):
    """The bf16 activation of a case, as fp32 on the CPU (every consumer starts from the same rounded values)."""
    return seeded_input(shape, 4300 + shape[1] + seed).to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------------------- GDFN case table
def tile(C, TH, TW, PC, NW, SAVE=False, F8=False):
    return ("tile", C, TH, TW, PC, NW, SAVE, F8)


def fourth(C, SAVE=False):
    return ("fourth", C, SAVE)


def _pair(inst, entry, cfg, shape, psets):
    return [(inst, entry, cfg, shape, p) for p in psets]


A, B_ = ("rb", "ew"), ("rw", "eb")         # each instance meets a ragged and an exact last chunk, bias on and off, both kinds
S48_16, S48_8, S96 = (2, 48, 32, 64), (2, 48, 24, 64), (2, 96, 24, 64)            # TW = 32: two tile columns, 2 / 3 / 3 tile rows
W48_16, W48_8, W96 = (2, 48, 32, 128), (2, 48, 24, 128), (2, 96, 24, 128)         # TW = 64
GDFN_CASES = (
    # inference, tile forms (FG_INFER_ROWS): C = 48 needs v2 (the default there is the fourth form)
    _pair(tile(48, 16, 32, 16, 4), "inference", "v2", S48_16, A) + _pair(tile(48, 8, 32, 16, 4), "inference", "v2", S48_8, B_)
    + _pair(tile(48, 8, 32, 32, 4), "inference", "v2,pc32", S48_8, A) + _pair(tile(96, 8, 32, 16, 4), "inference", "", S96, B_)
    + _pair(tile(96, 8, 32, 32, 4), "inference", "pc32", S96, A) + _pair(tile(48, 16, 64, 16, 8), "inference", "v2,w64", W48_16, B_)
    + _pair(tile(48, 8, 64, 32, 8), "inference", "v2,w64", W48_8, A) + _pair(tile(48, 8, 64, 16, 8), "inference", "v2,w64,pc16", W48_8, B_)
    + _pair(tile(96, 8, 64, 32, 8), "inference", "w64", W96, A) + _pair(tile(96, 8, 64, 16, 8), "inference", "w64,pc16", W96, B_)
    # inference, fourth form: the default at C = 48, v4 at C = 96; S = tiles / 2 at these sizes
    + _pair(fourth(48), "inference", "", S48_8, A) + _pair(fourth(96), "inference", "v4", S96, B_)
    # training (FG_TRAIN_ROWS, and the fourth form's SAVE kernels under v4); H = 24 reaches TH = 8 at C = 48 with no switch set
    + _pair(tile(48, 16, 32, 16, 4, SAVE=True), "train", "", S48_16, B_) + _pair(tile(48, 8, 32, 16, 4, SAVE=True), "train", "", S48_8, A)
    + _pair(tile(96, 8, 32, 16, 4, SAVE=True), "train", "", S96, B_) + _pair(tile(48, 16, 64, 16, 8, SAVE=True), "train", "w64", W48_16, A)
    + _pair(tile(96, 8, 64, 32, 8, SAVE=True), "train", "w64", W96, B_)
    + _pair(fourth(48, SAVE=True), "train", "v4", S48_8, B_) + _pair(fourth(96, SAVE=True), "train", "v4", S96, A)
    # fp8 operands (FG_F8_ROWS)
    + _pair(tile(48, 16, 32, 16, 4, F8=True), "f8", "", S48_16, A) + _pair(tile(48, 8, 32, 16, 4, F8=True), "f8", "", S48_8, B_)
    + _pair(tile(96, 8, 32, 16, 4, F8=True), "f8", "", S96, A)
    # launch-plan branches: a TW = 32 shape whose tile count is no multiple of 16 (no relabelling, default switches), the fourth
    # form with one persistent workgroup per image (two tiles) and with conv biases under a WithBias LayerNorm
    + [(tile(96, 8, 32, 16, 4), "inference", "", (1, 96, 24, 64), "rw"), (fourth(48), "inference", "", (2, 48, 8, 64), "rB")]
)
# xcd_pairs: 16 and 32 tiles, relabelled by default and not under MI_FG_NOXCD=1 - the outputs must be bit-identical
XCD_CASES = [(tile(96, 8, 32, 16, 4), (1, 96, 64, 64), "rw"), (tile(96, 8, 32, 16, 4), (2, 96, 64, 64), "eb"),
             (tile(48, 16, 32, 16, 4, SAVE=True), (2, 48, 64, 64), "rb")]
# fg4 persistent ranges: 256 / B binds (S = 4) and 10 tiles do not divide by it; the batch is copies of two distinct images
FG4_RANGES = (fourth(48), "", (52, 48, 40, 64), "rB", 4, 10)
# switch strings that leave an entry without an instance: (entry, cfg, shape, hidden)
GDFN_REFUSALS = [("train", "w64,pc16", (2, 96, 24, 128), 255), ("train", "pc32", (2, 96, 24, 64), 255),
                 ("train", "w64", (2, 48, 24, 128), 127), ("f8", "w64", (2, 96, 24, 128), 255), ("f8", "pc32", (2, 48, 24, 64), 127)]
GDFN_SWITCHES = sorted({c[2] for c in GDFN_CASES} | {r[1] for r in GDFN_REFUSALS} | {"v4,w64", "th8", "v2,th8"})


def case_id(case):
    inst, entry, cfg, shape, pset = case
    return "-".join([entry, "x".join(str(int(v)) if not isinstance(v, str) else v for v in inst), cfg or "default",
                     "x".join(map(str, shape)), pset])


def instance_of(plan):
    """The instance a plan names (None: not covered)."""
    if not plan["covered"]:
        return None
    if plan["family"] == "fourth":
        return fourth(plan["C"], plan["save"])
    return tile(plan["C"], plan["th"], plan["tw"], plan["pc"], plan["waves"], plan["save"], plan["f8"])


def set_switches(monkeypatch, cfg="", noxcd=False, fm_cfg=""):
    for name, val in (("MI_FG_CFG", cfg), ("MI_FG_NOXCD", "1" if noxcd else ""), ("MI_FM_CFG", fm_cfg)):
        if val:
            monkeypatch.setenv(name, val)
        else:
            monkeypatch.delenv(name, raising=False)
    for name in ("MI_FG_DEBUG", "MI_FM_DEBUG", "MI_NO_FUSED_MDTA"):
        monkeypatch.delenv(name, raising=False)


def reach(ops, inst, entry, shape, hidden):
    """Assert from the plan that this call, under the switches now set, runs `inst`; returns the plan."""
    p = ops.gdfn_fused_plan(shape, hidden, entry)
    assert instance_of(p) == inst, f"{entry} {shape} hidden {hidden}: the plan reaches {instance_of(p)}, the case is written for {inst}"
    tiles = p["tiles_x"] * p["tiles_y"]
    assert p["tiles_x"] >= 2 and p["tiles_y"] >= 1 and p["grid"] == shape[0] * p["S"] and 1 <= p["S"] <= tiles
    return p


def ladder_rows():
    """The (C, TH, TW, PC, NW) rows of the three dispatch lists, read from csrc/fused_gdfn.hip."""
    text = open(os.path.join(ROOT, "image_restoration_amd", "csrc", "fused_gdfn.hip")).read()
    out = {}
    for name, entry in (("FG_INFER_ROWS", "inference"), ("FG_TRAIN_ROWS", "train"), ("FG_F8_ROWS", "f8")):
        m = re.search(r"#define %s\(X\)((?:.*\\\n)*.*)\n" % name, text)
        rows = re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+)\)", m.group(1))
        assert rows, name
        out[entry] = [tuple(map(int, r)) for r in rows]
    return out


# ---------------------------------------------------------------------------------------------- MDTA case table
# kind, heads, MI_FM_CFG, form the plan must report
FM_KINDS = [("48_1", 48, 1, "", "fourth"), ("48_1", 48, 1, "v2", "round3"), ("96_2", 96, 2, "", "round3"), ("96_1", 96, 1, "", "round3")]
# shape without C, conv bias, LayerNorm kind, (tiles, S) the plan must report
FM_SHAPES = [((2, 24, 64), False, "WithBias", (6, 1)), ((1, 56, 64), True, "BiasFree", (14, 3)),      # 14 tiles over 3: ranges of 5, 5, 4
             ((3, 40, 128), True, "WithBias", (20, 5))]
MDTA_CASES = [(kind, C, heads, cfg, form, (s[0], C) + s[1:], bias, ln, ts)
              for kind, C, heads, cfg, form in FM_KINDS for s, bias, ln, ts in FM_SHAPES]
MDTA_REFUSALS = [((2, 192, 24, 64), 4), ((2, 48, 24, 32), 1), ((2, 96, 12, 64), 2), ((2, 96, 24, 64), 4)]   # shape, heads: no kind


def mdta_case_id(case):
    kind, C, heads, cfg, form, shape, bias, ln, ts = case
    return "-".join([kind, cfg or "default", form, "x".join(map(str, shape)), "bias" if bias else "nobias", ln])


# ---------------------------------------------------------------------------------------------- assertions
def errors(out, y, ref):
    """(error of out, error of the branch out - y) against the fp64 oracle, each of its tensor's largest magnitude."""
    y64 = y.detach().cpu().double()
    return rel(out, ref), rel(out.detach().cpu().double() - y64, ref.detach().cpu().double() - y64)


def assert_half_block(out, chain, y, ref, what=""):
    """The three bars of tests/test_gpu_fused.py on one half-block output.  -> (e_out, e_branch, e_chain)."""
    e_out, e_branch = errors(out, y, ref)
    e_chain = rel(chain, ref)
    print(f"{what}: out {e_out:.3e} branch {e_branch:.3e} chain {e_chain:.3e}")
    assert e_out < BAR_OUT, f"{what}: out off the fp64 oracle by {e_out:.3e} (chain {e_chain:.3e})"
    assert e_branch < BAR_BRANCH, f"{what}: branch off the fp64 oracle by {e_branch:.3e}"
    assert e_out < CHAIN_FACTOR * e_chain + CHAIN_SLACK, f"{what}: out {e_out:.3e} is further from the oracle than the chain {e_chain:.3e}"
    return e_out, e_branch, e_chain


def split_saved(saved, shape, hidden):
    """h0 [B, 2h, H, W] and g [B, h, H, W] out of the blob mi_gdfn_saved_bytes sizes (flags 0), as fp32."""
    B, _, H, W = shape
    n = B * hidden * H * W
    h0 = saved[: 4 * n].view(torch.bfloat16).float().view(B, 2 * hidden, H, W)
    off = (4 * n + 255) // 256 * 256
    return h0, saved[off: off + 2 * n].view(torch.bfloat16).float().view(B, hidden, H, W)


def oracle_h0(y, sd, kind):
    """project_in(LN(y)) in fp64."""
    d = {k: v.double() for k, v in sd.items()}
    yn = R.layernorm_nchw(y.double(), d["norm2.body.weight"], d.get("norm2.body.bias"), kind)
    return torch.nn.functional.conv2d(yn, d["ffn.project_in.weight"], d.get("ffn.project_in.bias"))


def assert_saved(h0, g, h0_chain, g_chain, h0_ref, what=""):
    e_h0, e_g, e_h0_ref = rel(h0, h0_chain), rel(g, g_chain), rel(h0, h0_ref)
    print(f"{what}: h0 vs chain {e_h0:.3e} g vs chain {e_g:.3e} h0 vs oracle {e_h0_ref:.3e} (chain's h0 {rel(h0_chain, h0_ref):.3e})")
    assert e_h0 < BAR_H0, f"{what}: saved h0 off the chain's by {e_h0:.3e}"
    assert e_g < BAR_G, f"{what}: saved g off the chain's by {e_g:.3e}"
    assert e_h0_ref < BAR_H0, f"{what}: saved h0 off the oracle's project_in(LN(y)) by {e_h0_ref:.3e}"
    return e_h0, e_g, e_h0_ref


def assert_pack_padding(pack, C, hidden, pc, out_w):
    """The tile sections of a pack (fg_pack_layout / fg_pack_kernel in csrc/fused_gdfn.hip), read back on the host: every
    entry of a pair past `hidden` in the last chunk - its W_in' rows and b', its W_out column, its depthwise taps and bias - and
    the row padding are exactly 0, and the W_out section holds bf16(W_out) everywhere else.  The padded pairs' g is 0 by the
    first and third, so no output can show a W_out column read past `hidden`: only this check does."""
    up = lambda v: -(-v // 256) * 256
    nch = -(-hidden // pc)
    blob = pack.detach().cpu()
    n1, n2, n3 = nch * 2 * pc * (C + 8), nch * C * (pc + 8), nch * pc * 20
    o2 = up(2 * n1)
    o3 = o2 + up(2 * n2)
    w1 = blob[: 2 * n1].view(torch.bfloat16).view(nch, 2, pc, C + 8).float()
    w2 = blob[o2: o2 + 2 * n2].view(torch.bfloat16).view(nch, C, pc + 8).float()
    wd = blob[o3: o3 + 4 * n3].view(torch.float32).view(nch, pc, 20)
    pad = (torch.arange(nch * pc) >= hidden).view(nch, pc)                           # pairs past the hidden width
    assert pad.sum() == nch * pc - hidden
    assert not w1[..., C + 2:].any(), "W_in' row padding is not zero"
    assert not w1.permute(0, 2, 1, 3)[pad].any(), "W_in' rows / b' of a pair past the hidden width are not zero"
    assert not wd[pad].any(), "depthwise taps / bias of a pair past the hidden width are not zero"
    assert not w2[..., pc:].any(), "W_out row padding is not zero"
    assert not w2.permute(0, 2, 1)[..., :pc, :][pad].any(), "W_out column of a pair past the hidden width is not zero"
    want = torch.zeros(nch * pc, C)
    want[:hidden] = out_w.detach().cpu().float().reshape(C, hidden).t().to(torch.bfloat16).float()
    assert torch.equal(w2[..., :pc].permute(0, 2, 1).reshape(nch * pc, C), want), "the W_out section is not bf16(W_out)"


# ---------------------------------------------------------------------------------------------- CPU model and injected faults
FAULTS = ("corner", "right_halo", "last_hidden", "padding", "swap")
FAULT_BAR = {"corner": "out", "right_halo": "out", "last_hidden": "out", "padding": "branch", "swap": "out"}   # the bar each must trip


def _bf(t, on):
    return t.to(torch.bfloat16).to(t.dtype) if on else t


def _gelu_bf16(x):
    """gelu_fwd<bf16> of csrc/common.h: x / (1 + 2^(x (-2.3083120 - 0.1004116 x^2)))."""
    return x / (1.0 + torch.exp2(x * (-2.3083120 - 0.1004116 * x * x)))


def model_half_block(y, sd, kind, mode, tile_hw=(8, 32), fault=None):
    """y + GDFN(LN(y)) on the CPU.  mode "fp64": the plain statement (with `fault`, the reference-only figure of what that fault
    costs).  mode "fused": the documented arithmetic of the fused kernels - fp32 accumulation, bf16 W_in diag(gamma), bf16
    normalised input, fp32 b' = b_in + W_in beta, bf16 h0 and g, gelu_fwd<bf16>, bf16 W_out and out.  mode "chain": the unfused
    chain - bf16 LN(y), bf16 W_in, and the rest alike.  tile_hw places the tile seams of the two halo faults.
    fault: "corner" - the halo pixel diagonally above-left of every tile that has one reads 0; "right_halo" - the column right of
    every tile that has one reads 0; "last_hidden" - project_out skips its last input channel; "padding" - h0 outside the image
    holds b' instead of 0; "swap" - the GELU goes to the second half of the gate."""
    F = torch.nn.functional
    q = mode != "fp64"
    dt = torch.float64 if mode == "fp64" else torch.float32
    d = {k: v.to(dt) for k, v in sd.items()}
    y = y.to(dt)
    Bn, C, H, W = y.shape
    gamma, beta = d["norm2.body.weight"], d.get("norm2.body.bias")
    w_in = d["ffn.project_in.weight"].reshape(-1, C)
    b_in, w_dw, b_dw = d.get("ffn.project_in.bias"), d["ffn.dwconv.weight"], d.get("ffn.dwconv.bias")
    w_out, b_out = d["ffn.project_out.weight"].reshape(C, -1), d.get("ffn.project_out.bias")
    h = w_out.shape[1]
    mu = y.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((y - mu) ** 2).mean(1, keepdim=True) + R.LN_EPS)
    xh = (y if kind == "BiasFree" else y - mu) * rstd
    bp = torch.zeros(2 * h, dtype=dt) if b_in is None else b_in.clone()          # b': what a zero LayerNorm input maps to
    if beta is not None:
        bp = bp + w_in @ beta
    if mode == "chain":
        yn = xh * gamma.view(1, -1, 1, 1) + (beta.view(1, -1, 1, 1) if beta is not None else 0.0)
        h0 = torch.einsum("mk,bkhw->bmhw", _bf(w_in, q), _bf(yn, q))
        if b_in is not None:
            h0 = h0 + b_in.view(1, -1, 1, 1)
    else:
        h0 = torch.einsum("mk,bkhw->bmhw", _bf(w_in * gamma.view(1, -1), q), _bf(xh, q)) + bp.view(1, -1, 1, 1)
    h0 = _bf(h0, q)
    if fault == "padding":
        hp = bp.view(1, -1, 1, 1).expand(Bn, 2 * h, H + 2, W + 2).clone()
        hp[:, :, 1:-1, 1:-1] = h0
    else:
        hp = F.pad(h0, (1, 1, 1, 1))
    t = F.conv2d(hp, w_dw, b_dw, groups=2 * h)
    TH, TW = tile_hw
    if fault == "corner":
        for y0 in range(TH, H, TH):
            for x0 in range(TW, W, TW):
                t[:, :, y0, x0] -= w_dw[:, 0, 0, 0] * h0[:, :, y0 - 1, x0 - 1]
    if fault == "right_halo":
        for x0 in range(TW, W, TW):                               # the column x0 is the right halo of the tiles left of it
            for ky in range(3):
                t[:, :, :, x0 - 1] -= w_dw[:, 0, ky, 2].view(1, -1, 1) * hp[:, :, ky: ky + H, x0 + 1]
    x1, x2 = (t[:, h:], t[:, :h]) if fault == "swap" else (t[:, :h], t[:, h:])
    g = _bf((_gelu_bf16(x1) if q else 0.5 * x1 * (1.0 + torch.erf(x1 / 2.0 ** 0.5))) * x2, q)
    wo = _bf(w_out, q).clone()
    if fault == "last_hidden":
        wo[:, h - 1] = 0
    out = y + torch.einsum("ck,bkhw->bchw", wo, g) + (b_out.view(1, -1, 1, 1) if b_out is not None else 0.0)
    return _bf(out, q), h0, g


def fault_table():
    """The distinct (C, parameter set, shape, tile) of the GDFN tables: what the fault check evaluates."""
    seen = []
    for inst, entry, cfg, shape, pset in list(GDFN_CASES) + [(i, "", "", s, p) for i, s, p in XCD_CASES]:
        thw = (8, 32) if inst[0] == "fourth" else (inst[2], inst[3])
        key = (shape[1], pset, (1,) + tuple(shape[1:]), thw)      # one image: the faults are per image
        if key not in seen:
            seen.append(key)
    return seen

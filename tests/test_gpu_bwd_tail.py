"""The backward tail (csrc/bwd_tail.hip: bt_kernel + bt_finish2_kernel) at every form, row tail and tile pass, against fp64.

Every case first asks ops.bwd_tail_plan (mi_bwd_tail_plan: the same bwd_tail_plan the launcher calls) and asserts the form,
the passes of the persistent loop and the waves that hold rows it was written for; tests/test_cabi.py::
test_tail_case_lists_reach_every_plan checks that the case lists below reach every form with one, two and three passes.

Family A - exact on integers.  The kernel takes mean and rstd as inputs, so every operand can be a small integer: x, dy, dres
  integer-valued bf16, mean an integer in [-1, 1] and rstd in {0.5, 1, 2} PER PIXEL (a statistic read for the wrong pixel or
  image changes the result), W in [-2, 3], gamma in {1, 2}, beta in [-1, 1].  Then xh = (x - mean) rstd and W gamma are exact
  in bf16 and every product and sum is a multiple of q = min(rstd, 1) in fp32.  The test asserts on the host that for every
  reduction (G = dY xh^T, S, dW, dgamma, dbeta, g = (W gamma)^T dY) the sum of the absolute values of its terms, in units of
  q, is below 2^24 and that |xh| <= 256: any summation order is then exact.  (The many-tile wide-M cases take the narrow
  ranges - dy, W in {-1, 0, 1}, x - mean in [-2, 2], rstd = 1 - for this to hold.)
      dW, dgamma, dbeta:  torch.equal with the fp64 statement cast to fp32 (accumulate: prefill + reference, integers too).
      dx, per element:    |dx - ref| <= 2^-8 |ref| + 2^-20 rstd (A + mean_c A + |xh| mean_c(A |xh|)),  A = sum_m |W gamma| |dy|:
                          the one bf16 rounding of the store, and the fp32 `* (1 / C)` and three-term combination of the
                          LayerNorm backward (an fp32 evaluation on the CPU reaches 0.996 of it).  No element is excluded.
Family B - real statistics (ops.ln_fwd), random float operands, modelled operand roundings.  The reference is fp64 arithmetic
  on the operands the kernel documents (model_operands): xh_b = bf16(fp32((x - mean) rstd)) and, for dx only,
  (W gamma)_b = bf16(fp32(W gamma)).  Per element, the worst-case fp32 summation bound, valid for any order:
      dW:             (B N + 16) 2^-24 (|gamma| sum |dy| |xh_b| + |beta| sum |dy|)
      dgamma, dbeta:  (B N + M + 16) 2^-24 sum_m |W| (that row's abs-sum)
      dx:             2^-8 |ref| + (M + C + 16) 2^-24 rstd (A + mean_c A + |xh_b| mean_c(A |xh_b|))
  and the modelled reference itself lies within the 2e-2 / 1e-2 max-norm bars of the pure fp64 statement.

Worst err / bound seen on an MI355X (informational; the bounds are derived, not fitted): see DESIGN.md, backward tail.

The module imports without a GPU: evaluate_fp32 (the tail in torch fp32 on the CPU, in a permuted summation order, with
optional deliberate faults) goes through the same assertion helpers in tests/test_cabi.py, which shows that the bounds admit
a correct evaluation and that the assertions catch a dropped row, swapped statistics, a stale dres tile and a doubled partial.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle.fixtures import seeded_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SWITCHES = ("MI_BT_DEBUG", "MI_BT_WIDE")
FORMS = {(48, 3): (4, 512), (48, 4): (4, 512), (96, 3): (8, 256), (96, 4): (8, 256)}   # (C, fragments per wave): waves, grid
MAX_NORM_DX, MAX_NORM_PARAM = 2e-2, 1e-2      # the bars of tests/test_gpu_fused.py::test_bwd_tail_vs_fp64

# --------------------------------------------------------------------------- case lists
# A case: (C, fragments, M, B, tiles per image, passes, dres given, accumulate, narrow ranges)
ROW_MS = {(48, 3): (16, 17, 47, 48, 49, 97, 144, 191, 192), (48, 4): (193, 254, 255, 256),
          (96, 3): (16, 17, 49, 288, 383, 384), (96, 4): (385, 449, 510, 512)}
# every row count at B = 2 on a 9-tile plane (8 x 72), dres given; accumulate alternates
ROW_CASES = [(C, f, M, 2, 9, 1, True, i % 2 == 1, False) for (C, f), ms in ROW_MS.items() for i, M in enumerate(ms)]

SMALL_M = {(48, 3): 17, (48, 4): 193, (96, 3): 49, (96, 4): 385}
WIDE_M = {(48, 3): 191, (48, 4): 254, (96, 3): 383, (96, 4): 510}
# grid + 1 and 2 grid + 1 tiles as (B, tiles per image): a workgroup's successive tiles fall in different images at different offsets
OVER = {48: ((27, 19), (205, 5)), 96: ((1, 257), (27, 19))}


def _tile_cases():
    out = []
    for (C, f) in FORMS:
        m, many = SMALL_M[(C, f)], f == 4                  # the 4-fragment forms have no small M: narrow ranges over many tiles
        out += [(C, f, m, 1, 1, 1, True, False, False),    # one tile
                (C, f, m, 3, 1, 1, True, True, False),     # every tile another image
                (C, f, m) + OVER[C][0] + (2, True, False, many),      # one workgroup takes a second tile while the rest end
                (C, f, m) + OVER[C][1] + (3, True, True, many),       # a third pass: the double buffers are reused
                (C, f, WIDE_M[(C, f)]) + OVER[C][1] + (3, True, False, True)]
    return out


TILE_CASES = _tile_cases()
# dres == nullptr (dx is the LayerNorm backward alone): every form, one pass and three, accumulate on and off
OPTION_CASES = ([(C, f, WIDE_M[(C, f)], 2, 9, 1, False, C == 48, False) for (C, f) in FORMS] +
                [(C, f, SMALL_M[(C, f)]) + OVER[C][1] + (3, False, C == 96, f == 4) for (C, f) in FORMS])
EXACT_CASES = ROW_CASES + TILE_CASES + OPTION_CASES

# Family B: (C, fragments, M, B, tiles per image), B N <= 2048, each with a row tail
MODEL_CASES = [(48, 3, 190, 2, 9), (48, 4, 254, 3, 9), (96, 3, 383, 2, 16), (96, 4, 510, 3, 7)]


def case_id(c):
    C, f, M, B, tpi = c[:5]
    tail = "" if len(c) == 5 else f"-p{c[5]}-{'dres' if c[6] else 'nodres'}-{'acc' if c[7] else 'set'}{'-narrow' if c[8] else ''}"
    return f"C{C}x{f}-M{M}-B{B}-t{tpi}{tail}"


def ops():
    from image_restoration_amd import ops as o
    return o


def expected_plan(C, f, M, tiles):
    """(waves, fragments, workgroups, passes, active waves) of a case, from the table of the kernel's forms."""
    waves, grid = FORMS[(C, f)]
    wgs = min(tiles, grid)
    return waves, f, wgs, -(-tiles // wgs), -(-M // (16 * f))


def assert_plan(C, f, M, B, tpi, passes=None):
    """The plan of the call is the one the case was written for; -> the plan."""
    p = ops().bwd_tail_plan(M, C, B, 64 * tpi, BF16)
    want = expected_plan(C, f, M, B * tpi)
    assert p["covered"] and (p["waves"], p["fragments"], p["workgroups"], p["passes"], p["active_waves"]) == want, (p, want)
    assert passes is None or p["passes"] == passes, (p, passes)
    return p


# --------------------------------------------------------------------------- inputs (CPU tensors)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_inputs(C, M, B, tpi, dres=True, narrow=False):
    """Family A operands: see the module docstring."""
    N, g = 64 * tpi, _gen(7919 * M + 104729 * C + 31 * B + tpi + (1 << 20) * narrow)
    s = SimpleNamespace(C=C, M=M, B=B, tpi=tpi, N=N)
    s.mean = _ints(-1, 1, (B, N), g)
    s.rstd = torch.ones(B, N) if narrow else torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (B, N), generator=g)]
    d = _ints(-2, 2, (B, C, N), g) if narrow else _ints(-3, 3, (B, C, N), g)            # x - mean
    s.x = (d + s.mean[:, None, :]).to(BF16)
    s.dy = (_ints(-1, 1, (B, M, N), g) if narrow else _ints(-2, 2, (B, M, N), g)).to(BF16)
    s.dres = _ints(-4, 4, (B, C, N), g).to(BF16) if dres else None
    s.w = _ints(-1, 1, (M, C), g) if narrow else _ints(-2, 3, (M, C), g)
    s.gamma = _ints(1, 2, (C,), g)
    s.beta = _ints(-1, 1, (C,), g)
    return s


def float_inputs(C, M, B, tpi, stats=None):
    """Family B operands, scaled as in tests/test_gpu_fused.py::test_bwd_tail_vs_fp64.  stats: None (filled by the caller from
    ops.ln_fwd) or "cpu" (fp32 statistics computed here, for the host-only tests)."""
    N, seed = 64 * tpi, 100 * M + C
    s = SimpleNamespace(C=C, M=M, B=B, tpi=tpi, N=N)
    s.x = (seeded_input((B, C, N), seed) * 1.5 + 0.3).to(BF16)
    s.dy = seeded_input((B, M, N), seed + 1).to(BF16)
    s.dres = seeded_input((B, C, N), seed + 2).to(BF16)
    s.w = (seeded_input((M, C), seed + 3) * 0.2).float().contiguous()
    s.gamma = (1.0 + 0.3 * seeded_input((C,), seed + 4)).float()
    s.beta = (0.2 * seeded_input((C,), seed + 5)).float()
    if stats == "cpu":
        xf = s.x.float()
        s.mean = xf.mean(1)
        s.rstd = 1.0 / torch.sqrt(xf.var(1, unbiased=False) + 1e-5)
    return s


# --------------------------------------------------------------------------- the fp64 reference
def _flat(t):
    """[B, R, N] -> [R, B N] in fp64."""
    return t.double().permute(1, 0, 2).reshape(t.shape[1], -1)


def _unflat(t, B):
    """[R, B N] -> [B, R, N]."""
    return t.reshape(t.shape[0], B, -1).permute(1, 0, 2).contiguous()


def model_operands(s):
    """The two operand roundings the kernel documents, as fp64 values: xh_b = bf16((x - mean) rstd), computed in fp32 from the
    fp32 statistics it was handed (bwd_tail.hip:363), and (W gamma)_b = bf16(W gamma), an fp32 product (bwd_tail.hip:128),
    which enters dx only.  A kernel that moves a rounding point changes THIS helper, not a tolerance."""
    xh = ((s.x.float() - s.mean[:, None, :]) * s.rstd[:, None, :]).to(BF16)
    wg = (s.w * s.gamma[None, :]).to(BF16)
    return _flat(xh), wg.double()


def exact_operands(s):
    """xh and W gamma in fp64 from the statistics supplied (Family A: these ARE the kernel's bf16 operands)."""
    return (_flat(s.x) - s.mean.double().reshape(1, -1)) * s.rstd.double().reshape(1, -1), s.w.double() * s.gamma.double()[None, :]


def pure_operands(s):
    """The operation itself: fp64 statistics of x (WithBias_LayerNorm, eps 1e-5), no operand rounding."""
    x = _flat(s.x).reshape(s.C, s.B, s.N)
    mu = x.mean(0, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var(0, unbiased=False, keepdim=True) + 1e-5)
    return ((x - mu) * rstd).reshape(s.C, -1), s.w.double() * s.gamma.double()[None, :], rstd.reshape(-1)


def reference(s, xh, wg, rstd=None):
    """fp64 statement of the tail on the given xh [C, B N] and W gamma [M, C] (the math of _tail_reference in
    tests/test_gpu_fused.py), with the abs-sums of every reduction that the preconditions and bounds need."""
    dy, w, gamma, beta = _flat(s.dy), s.w.double(), s.gamma.double(), s.beta.double()
    rstd = s.rstd.double().reshape(-1) if rstd is None else rstd
    r = SimpleNamespace()
    G, S = dy @ xh.T, dy.sum(1)
    r.dw = gamma[None, :] * G + beta[None, :] * S[:, None]
    r.dgamma, r.dbeta = (w * G).sum(0), (w * S[:, None]).sum(0)
    g = wg.T @ dy
    dx = rstd * (g - g.mean(0) - xh * (g * xh).mean(0))
    r.dx = _unflat(dx + (_flat(s.dres) if s.dres is not None else 0.0), s.B)
    # abs-sums
    ady, axh = dy.abs(), xh.abs()
    r.aG, r.aS = ady @ axh.T, ady.sum(1)
    r.a_dw = gamma.abs()[None, :] * r.aG + beta.abs()[None, :] * r.aS[:, None]
    r.a_dgamma, r.a_dbeta = (w.abs() * r.aG).sum(0), (w.abs() * r.aS[:, None]).sum(0)
    r.A = wg.abs().T @ ady
    r.dx_slack = _unflat(rstd * (r.A + r.A.mean(0) + axh * (r.A * axh).mean(0)), s.B)
    r.xh_max = float(axh.max())
    r.q = min(float(rstd.min()), 1.0)
    return r


def assert_exact_preconditions(s, r, prefill=0.0):
    """Any summation order is exact: every term is a multiple of q and each reduction's abs-sum in units of q is below 2^24."""
    assert r.xh_max <= 256
    for name in ("aG", "aS", "a_dw", "a_dgamma", "a_dbeta", "A"):
        worst = (float(getattr(r, name).max()) + abs(prefill)) / r.q
        assert worst < 2 ** 24, (name, worst, case_id((s.C, 0, s.M, s.B, s.tpi)))


@functools.lru_cache(maxsize=2)
def exact_case(C, M, B, tpi, dres, narrow):
    s = exact_inputs(C, M, B, tpi, dres, narrow)
    r = reference(s, *exact_operands(s))
    assert_exact_preconditions(s, r, prefill=max(abs(v) for v in PREFILL.values()))
    return s, r


# --------------------------------------------------------------------------- assertions (shared with the CPU tests)
PREFILL = {"dw": 3.0, "dgamma": -2.0, "dbeta": 5.0}


def _where(s, plan, b, c, p):
    """Which tile, pass and workgroup wrote dx[b, c, p]."""
    tile = b * s.tpi + p // 64
    return f"image {b} channel {c} pixel {p}: tile {tile} = pass {tile // plan['workgroups']} of workgroup {tile % plan['workgroups']}"


def assert_dx(got, ref, bound, s, plan, what):
    """Per element |got - ref| <= bound, no element excluded; -> worst err / bound."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)                                   # a NaN is bad
    if bool(bad.any()):
        b, c, p = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: dx off at {int(bad.sum())} of {bad.numel()} elements, first at {_where(s, plan, b, c, p)}: "
                             f"got {float(got[b, c, p])}, want {float(ref[b, c, p])}, bound {float(bound[b, c, p]):.3e}")
    return float((err / bound.clamp_min(1e-300)).max())


def assert_param_equal(got, want, s, plan, name, what):
    want = want.float()
    if not torch.equal(got, want):
        bad = (got != want) | got.isnan()
        idx = tuple(int(v) for v in bad.nonzero()[0])
        rows = f" (row {idx[0]}: fragment {idx[0] // 16 % plan['fragments']} of wave {idx[0] // plan['rows_per_wave']})" if name == "dw" else ""
        raise AssertionError(f"{what}: {name} differs at {int(bad.sum())} of {bad.numel()} elements, first at {idx}{rows}: "
                             f"got {float(got[idx])}, want {float(want[idx])}")


def assert_exact(got, s, r, plan, accumulate, what):
    """Family A: got = (dx [B, C, N] bf16, dw, dgamma, dbeta fp32) on the CPU.  -> (worst dx err / bound, share of dx bit-equal
    to bf16(ref))."""
    dx, dw, dgamma, dbeta = got
    for name, g_, w_ in (("dw", dw, r.dw), ("dgamma", dgamma, r.dgamma), ("dbeta", dbeta, r.dbeta)):
        assert_param_equal(g_, w_ + (PREFILL[name] if accumulate else 0.0), s, plan, name, what)
    bound = 2.0 ** -8 * r.dx.abs() + 2.0 ** -20 * r.dx_slack
    ratio = assert_dx(dx, r.dx, bound, s, plan, what)
    return ratio, float((dx == r.dx.to(BF16)).double().mean())


def assert_model(got, s, r, plan, what):
    """Family B: got as above against the modelled reference, worst-case fp32 summation bounds.  -> worst err / bound of
    (dx, dw, dgamma, dbeta)."""
    dx, dw, dgamma, dbeta = got
    u, P = 2.0 ** -24, s.B * s.N
    ratios = [assert_dx(dx, r.dx, 2.0 ** -8 * r.dx.abs() + (s.M + s.C + 16) * u * r.dx_slack, s, plan, what)]
    for name, g_, w_, bound in (("dw", dw, r.dw, (P + 16) * u * r.a_dw), ("dgamma", dgamma, r.dgamma, (P + s.M + 16) * u * r.a_dgamma),
                                ("dbeta", dbeta, r.dbeta, (P + s.M + 16) * u * r.a_dbeta)):
        err = (g_.double() - w_).abs()
        bad = ~(err <= bound)
        if bool(bad.any()):
            idx = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{what}: {name} off at {int(bad.sum())} of {bad.numel()} elements, first at {idx}: got {float(g_[idx])}, "
                                 f"want {float(w_[idx])}, bound {float(bound[idx]):.3e}")
        ratios.append(float((err / bound.clamp_min(1e-300)).max()))
    return ratios


def max_norm(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def assert_model_near_statement(s, r):
    """The modelled reference has not wandered from the operation: within the max-norm bars of the pure fp64 statement."""
    xh, wg, rstd = pure_operands(s)
    p = reference(s, xh, wg, rstd)
    assert max_norm(r.dx, p.dx) < MAX_NORM_DX
    for name in ("dw", "dgamma", "dbeta"):
        assert max_norm(getattr(r, name), getattr(p, name)) < MAX_NORM_PARAM, name
    return p


# --------------------------------------------------------------------------- the tail in torch fp32 on the CPU
FAULTS = ("drop_last_row", "swap_rstd", "stale_dres", "double_partial")


def evaluate_fp32(s, workgroups, accumulate=False, fault=None, seed=0):
    """What the kernels compute, in fp32 on the CPU with the bf16 operand roundings of model_operands, per-workgroup partials of
    [G | S] over tiles dealt round-robin, and every sum in a permuted order.  fault: one of FAULTS, a deliberate error of the
    kind the GPU tests exist to catch.  -> (dx, dw, dgamma, dbeta) like the GPU call."""
    g = _gen(seed)
    C, M, B, P = s.C, s.M, s.B, s.B * s.N
    T = P // 64
    wgs = min(T, workgroups)
    f32 = lambda t: _flat(t).float()
    rstd, mean = s.rstd.reshape(-1).clone(), s.mean.reshape(-1)
    if fault == "swap_rstd":                                # two pixels of the last tile with different statistics
        lo = 64 * (T - 1)
        j = next(j for j in range(lo + 1, lo + 64) if rstd[j] != rstd[lo])
        rstd[[lo, j]] = rstd[[j, lo]]
    xh = ((f32(s.x) - mean) * rstd).to(BF16).float()
    wg = (s.w * s.gamma[None, :]).to(BF16).float()
    dy = f32(s.dy)
    # partials [G | S] per workgroup, tiles in a shuffled order
    dyt, xht = dy.reshape(M, T, 64).permute(1, 0, 2), xh.reshape(C, T, 64).permute(1, 0, 2)
    per_tile = torch.cat([dyt @ xht.transpose(1, 2), dyt.sum(2, keepdim=True)], 2)            # [T, M, C + 1]
    order = torch.randperm(T, generator=g)
    part = torch.zeros(wgs, M, C + 1).index_add_(0, order % wgs, per_tile[order])
    total = part[torch.randperm(wgs, generator=g)].sum(0)
    if fault == "double_partial":
        total = total + part[wgs - 1]
    gg, ss = total[:, :C], total[:, C:]
    pre = {k: (v if accumulate else 0.0) for k, v in PREFILL.items()}
    rows = torch.randperm(M, generator=g)
    dw = pre["dw"] + s.gamma[None, :] * gg + s.beta[None, :] * ss
    dgamma = pre["dgamma"] + (s.w * gg)[rows].sum(0)
    dbeta = pre["dbeta"] + (s.w * ss)[rows].sum(0)
    # dxn over shuffled rows, LayerNorm backward over shuffled channels
    if fault == "drop_last_row":
        rows = rows[rows != M - 1]
    gx = wg[rows].T @ dy[rows]
    ch, inv_c = torch.randperm(C, generator=g), torch.tensor(1.0 / C, dtype=torch.float32)
    s1, s2 = gx[ch].sum(0) * inv_c, (gx * xh)[ch].sum(0) * inv_c
    o = rstd * (gx - s1 - xh * s2)
    dres = f32(s.dres).clone() if s.dres is not None else torch.zeros(C, P)
    if fault == "stale_dres":                               # the last tile gets the dres of its workgroup's tile two passes back
        back = 2 * wgs if T > 2 * wgs else 2
        dres[:, 64 * (T - 1):] = dres[:, 64 * (T - 1 - back):64 * (T - back)]
    return _unflat((o + dres).to(BF16), B), dw, dgamma, dbeta


# --------------------------------------------------------------------------- the GPU call
@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _dev4(t, s):
    return None if t is None else t.reshape(s.B, t.shape[1], 8, s.N // 8).to(DEV).contiguous()


def device_operands(s):
    d = SimpleNamespace(x=_dev4(s.x, s), dy=_dev4(s.dy, s), dres=_dev4(s.dres, s), w=s.w.to(DEV), gamma=s.gamma.to(DEV), beta=s.beta.to(DEV))
    d.mean, d.rstd = (s.mean.to(DEV), s.rstd.to(DEV)) if hasattr(s, "mean") else (None, None)
    return d


def run_tail(s, d, accumulate):
    """One ops.bwd_tail call; overwrite mode starts from NaN-filled gradients, accumulate from PREFILL.  -> CPU tensors."""
    fill = (lambda k: PREFILL[k]) if accumulate else (lambda k: float("nan"))
    dw = torch.full((s.M, s.C), fill("dw"), device=DEV)
    dgamma, dbeta = torch.full((s.C,), fill("dgamma"), device=DEV), torch.full((s.C,), fill("dbeta"), device=DEV)
    dx = ops().bwd_tail(d.dy, d.x, d.dres, d.mean, d.rstd, d.w, d.gamma, d.beta, dw, dgamma, dbeta, accumulate)
    torch.cuda.synchronize()
    return dx.reshape(s.B, s.C, s.N).cpu(), dw.cpu(), dgamma.cpu(), dbeta.cpu()


# --------------------------------------------------------------------------- Family A
@pytest.mark.parametrize("case", EXACT_CASES, ids=case_id)
def test_tail_exact_on_integers(case):
    C, f, M, B, tpi, passes, dres, accumulate, narrow = case
    plan = assert_plan(C, f, M, B, tpi, passes)
    s, r = exact_case(C, M, B, tpi, dres, narrow)
    got = run_tail(s, device_operands(s), accumulate)
    ratio, equal = assert_exact(got, s, r, plan, accumulate, case_id(case))
    print(f"tail exact {case_id(case)}: dx worst err/bound {ratio:.3f}, bit-equal to bf16(ref) {100 * equal:.2f} %")


@pytest.mark.parametrize("C,f", list(FORMS), ids=lambda v: str(v))
def test_tail_small_call_after_three_passes_reads_no_stale_partial(C, f):
    """bt_finish2_kernel sums min(tiles, grid) partials out of a workspace that is reused: a one-tile call right after a
    three-pass call of the same (M, C) must not see what the large call left there."""
    M = SMALL_M[(C, f)]
    (Bb, tb), narrow = OVER[C][1], f == 4
    big, small = exact_case(C, M, Bb, tb, True, narrow), exact_case(C, M, 1, 1, True, narrow)
    pb, ps = assert_plan(C, f, M, Bb, tb, 3), assert_plan(C, f, M, 1, 1, 1)
    db, dsm = device_operands(big[0]), device_operands(small[0])
    got_big = run_tail(big[0], db, False)
    got_small = run_tail(small[0], dsm, False)
    assert_exact(got_big, *big, pb, False, "three passes")
    assert_exact(got_small, *small, ps, False, "one tile after three passes")


@pytest.mark.parametrize("C,f", list(FORMS), ids=lambda v: str(v))
def test_tail_is_deterministic(C, f):
    """Partials are per workgroup and summed in a fixed order: two calls on the same inputs agree bit for bit."""
    M, (B, tpi) = WIDE_M[(C, f)], OVER[C][0]
    assert_plan(C, f, M, B, tpi, 2)
    s = float_inputs(C, M, B, tpi, stats="cpu")
    d = device_operands(s)
    a, b = run_tail(s, d, False), run_tail(s, d, False)
    for name, u, v in zip(("dx", "dw", "dgamma", "dbeta"), a, b):
        assert torch.equal(u.view(torch.int16) if u.dtype == BF16 else u.view(torch.int32),
                           v.view(torch.int16) if v.dtype == BF16 else v.view(torch.int32)), name


def test_tail_rejects_misaligned_and_uncovered_calls_before_any_launch():
    """A statistic or activation pointer off the 16-byte grid, a row count past the last form and a pixel count that is no
    multiple of the tile: the library's error from the host-side check, and no output touched."""
    o = ops()
    s = exact_inputs(96, 49, 2, 2)
    d = device_operands(s)

    def off_by_one(t):                                      # the same values one element past a 16-byte boundary
        return torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)[1:1 + t.numel()].copy_(t.reshape(-1)).view(t.shape)

    def refused(match, **kw):
        a = {**vars(d), **kw}
        dw, dgamma, dbeta = (torch.full(sh, 7.0, device=DEV) for sh in ((a["dy"].shape[1], 96), (96,), (96,)))
        with pytest.raises(RuntimeError, match=match):
            o.bwd_tail(a["dy"], a["x"], a["dres"], a["mean"], a["rstd"], a["w"], a["gamma"], a["beta"], dw, dgamma, dbeta, False)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in (dw, dgamma, dbeta))

    for name in ("mean", "x"):
        t = off_by_one(getattr(d, name))
        assert t.data_ptr() % 16 != 0 and t.is_contiguous()
        refused("16-byte aligned", **{name: t})
    assert not o.bwd_tail_plan(513, 96, 2, 128, BF16)["covered"] and not o.bwd_tail_plan(49, 96, 2, 96, BF16)["covered"]
    refused("unsupported shape", dy=torch.zeros(2, 513, 8, 16, dtype=BF16, device=DEV), w=torch.zeros(513, 96, device=DEV))
    z = lambda r: torch.zeros(2, r, 8, 12, dtype=BF16, device=DEV)
    refused("unsupported shape", dy=z(49), x=z(96), dres=z(96), mean=torch.zeros(2, 96, device=DEV), rstd=torch.ones(2, 96, device=DEV))


# --------------------------------------------------------------------------- Family B
@pytest.mark.parametrize("case", MODEL_CASES, ids=case_id)
def test_tail_real_statistics_against_modelled_operands(case):
    C, f, M, B, tpi = case
    plan = assert_plan(C, f, M, B, tpi, 1)
    assert M % 16 != 0 and B * 64 * tpi <= 2048
    s = float_inputs(C, M, B, tpi)
    d = device_operands(s)
    _, d.mean, d.rstd = ops().ln_fwd(d.x, d.gamma, d.beta, True, want_stats=True)
    s.mean, s.rstd = d.mean.cpu(), d.rstd.cpu()
    r = reference(s, *model_operands(s))
    assert_model_near_statement(s, r)
    ratios = assert_model(run_tail(s, d, False), s, r, plan, case_id(case))
    print(f"tail model {case_id(case)}: worst err/bound dx {ratios[0]:.3f} dw {ratios[1]:.3f} dgamma {ratios[2]:.3f} dbeta {ratios[3]:.3f}")

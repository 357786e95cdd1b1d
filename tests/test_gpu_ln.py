"""Channel LayerNorm (csrc/ln.hip) over every kernel form, channel bin, pixel tail and alignment, against the fp64 oracle
(oracle.restormer_ref.layernorm_nchw and its autograd) evaluated on the inputs AS STORED: bf16 inputs are rounded first and
then widened, so storage rounding of the inputs is not counted as kernel error.

Every case asks ops.ln_plan (mi_ln_plan: the same ln_fwd_plan / ln_bwd_plan the launchers call) what runs and asserts that
it is the form the case was written for; tests/test_cabi.py::test_ln_case_lists_reach_every_plan enumerates the plans the
dispatch can produce and checks that the case lists below (CHANNEL_CASES, PIXEL_CASES, MISALIGNED) reach each of them.

Bounds
  y, dx (dx includes dres), per element:  fp32 |got - ref| <= 2e-5 max|ref|;  bf16 <= 2^-8 |ref| + 2e-5 max|ref| (one bf16
      unit of the stored result - round-to-nearest costs half a unit and fp32 noise may move a value across one rounding
      boundary - plus the fp32 bound as the floor for elements that are small by cancellation).
  mean, rstd:  2e-5 of max|x| and of max|rstd|.
  dbeta:  EXACT.  dy holds integers in [-3, 3] and B * N * 3 < 2^24, so every partial and every total is an integer that
      fp32 holds whatever the summation order, in both dtypes: torch.equal with the integer sum.  Any lost, doubled or
      misplaced pixel, tile, image or partial row - in the LN kernels, in reduce_rows_kernel (both stages) and in
      deferred_reduce_kernel - changes it.  Prior values of db in the accumulate cases are integers too.
  dgamma:  per channel, |got - ref| <= bound * S_c with S_c = sum |dy * xhat| in fp64 (xhat = x * rstd for BiasFree).
      The bound does not come from the kernel: the same oracle evaluated in fp32 on the CPU at the same inputs
      (measure_fp32_oracle below) has a worst normalised error of 3.79e-4 over CHANNEL_CASES + PIXEL_CASES + TWO_STAGE.
      The GPU sums in another order (wave tree, partial rows, one or two row stages) and is allowed 4x that: 1.52e-3.
      That worst case is a single pixel (B * N = 1), where S_c is one term and x - mu of a channel may cancel to 1e-4 of
      |x|; it says little about a sum over pixels, so the bound is taken per class of pixel count, each from the
      oracle's worst error over the cases of that class, which is never looser:
          B * N = 1       measured 3.79e-4   bound 1.52e-3
          B * N = 2..63   measured 2.45e-6   bound 9.8e-6
          B * N >= 64     measured 4.89e-8   bound 1.96e-7
      The ill-conditioned inputs (x = 50 + 0.5 randn, B * N = 260) have their own figure, measured the same way:
      1.40e-6, bound 5.6e-6.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle import restormer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTS = {"f32": F32, "bf16": BF16}
FLOOR = 2e-5                       # the project's fp32 bound (TOL in tests/test_gpu_primitives.py)
BF16_UNIT = 2.0 ** -8
DGAMMA_ORACLE_F32 = ((1, 3.79e-4), (63, 2.45e-6), (1 << 62, 4.89e-8))   # (pixels up to, measured): see the module docstring
DGAMMA_ORACLE_F32_ILL = 1.40e-6
DGAMMA_BOUND_ILL = 4 * DGAMMA_ORACLE_F32_ILL
F32_ADD = 2.0 ** -23               # one fp32 rounding of prior + gradient (accumulate cases), relative to the sum
ILL_OFFSET = 50.0

FORMS = ("default", "wave", "block")

# --------------------------------------------------------------------------- case lists: (B, C, N, dtype, with_bias, form)
CH_C = (1, 2, 15, 16, 17, 24, 25, 47, 48, 49, 95, 96, 97, 191, 192, 193, 383, 384, 385, 767, 768)
CH_BN = ((1, 1), (3, 65), (2, 130))
# "other" = every forced MI_LN_FORM (wave, block) that changes the plan of the call: the default plus these are all three forms
CHANNEL_CASES = [(B, C, N, d, wb, f) for C in CH_C for (B, N) in CH_BN for d in ("f32", "bf16") for wb in (True, False)
                 for f in ("default", "other")]

PX_N = (1, 2, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 513)
PX_C = (16, 48, 96, 192, 384, 768)
# the bias kind alternates over the grid
PIXEL_CASES = [(3, C, N, d, (i + j) % 2 == 0, f) for j, C in enumerate(PX_C) for i, N in enumerate(PX_N)
               for d in ("f32", "bf16") for f in ("default", "other")]

# bf16, even N, ONE operand carved at an odd element offset: (B, C, N, operand)
MISALIGNED = [(2, C, 130, op) for C in (16, 48, 96, 192, 384) for op in ("x_fwd", "dy", "x", "dres")]

# rows = tiles * B: 44 * 3 = 132 > 128 takes the two-stage reduction, 64 * 2 = 128 is the last single-stage count
TWO_STAGE = [(3, 16, 2753, True), (3, 96, 2753, True), (2, 16, 4033, False), (2, 96, 4033, False)]


def case_id(c):
    B, C, N, d, wb, f = c
    return f"C{C}-B{B}-N{N}-{d}-{'bias' if wb else 'nobias'}-{f}"


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def ops():
    from image_restoration_amd import ops as o
    return o


def lib():
    from image_restoration_amd import _lib
    return _lib


# --------------------------------------------------------------------------- plans
def plan_key(direction, d, pl):
    """A plan without the parts that follow the pixel count: one key per kernel instance."""
    return (direction, d) + tuple(sorted((k, v) for k, v in pl.items() if k not in ("gx", "rows", "two_stage")))


def plans(B, C, N, d, aligned=True):
    o = ops()
    return o.ln_plan(B, C, N, DTS[d], False, aligned), o.ln_plan(B, C, N, DTS[d], True, aligned)


def capacity(pl):
    return pl["CB"] * pl["WS"] if pl["family"] == "wave" else pl["waves"] * pl["CPT"]


def set_form(monkeypatch, form):
    """MI_LN_FORM for this test (the conftest fixture reloads the library's switches now and restores them afterwards)."""
    if form == "default":
        monkeypatch.delenv("MI_LN_FORM", raising=False)
    else:
        monkeypatch.setenv("MI_LN_FORM", form)


def resolve_form(monkeypatch, B, C, N, d, form):
    """The forms to run for `form` as [(MI_LN_FORM value, fwd plan, bwd plan)]; setting a switch that changes nothing for
    this call is left out (the default case already runs those kernels), so the list may be empty.  'other' stands for every
    forced form that differs from the default: one below C = 384, both at C = 384 (forward block, backward wave-owned)."""
    set_form(monkeypatch, "default")
    base = plans(B, C, N, d)
    if form == "default":
        return [("default",) + base]
    out = []
    for f in (("wave", "block") if form == "other" else (form,)):
        set_form(monkeypatch, f)
        forced = plans(B, C, N, d)
        if forced != base:
            assert f in (forced[0]["family"], forced[1]["family"]), (f, forced)
            out.append((f,) + forced)
    return out


def run_forms(monkeypatch, todo, fn):
    for f, pf, pb in todo:
        set_form(monkeypatch, f)
        fn(f, pf, pb)


def reached_plans(monkeypatch):
    """Every plan key the case lists of this file run (host-only: used by the coverage test in tests/test_cabi.py)."""
    seen = set()
    for B, C, N, d, _, f in CHANNEL_CASES + PIXEL_CASES:
        for _, pf, pb in resolve_form(monkeypatch, B, C, N, d, f):
            seen.update({plan_key("fwd", d, pf), plan_key("bwd", d, pb)})
    set_form(monkeypatch, "default")
    for B, C, N, op in MISALIGNED:
        pf, pb = plans(B, C, N, "bf16", aligned=False)
        seen.add(plan_key("fwd", "bf16", pf) if op == "x_fwd" else plan_key("bwd", "bf16", pb))
    return seen


# --------------------------------------------------------------------------- inputs and the fp64 reference (CPU, cached)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_inputs(B, C, N, d, wb, data="plain"):
    dt = DTS[d]
    seed = 1000003 * C + 1009 * N + 17 * B + (1 if wb else 0)
    shape = (B, C, 1, N)
    if data == "plain":
        x = torch.randn(shape, generator=_gen(seed)) * 1.5 + 0.3
        # A pixel whose channels nearly tie (likely at C = 2, 3) has rstd up to 316 and x - mu cancels: the oracle itself,
        # evaluated in fp32, then misses the fp32 bound of dx by 5-8x (measured at C = 2).  That is the data's condition, not
        # a kernel's error, so such pixels are spread by +-1 over alternating channels; variance 0 has its own test below.
        tie = x.std(dim=1, unbiased=False, keepdim=True) < 0.5 if C > 1 else torch.zeros_like(x[:, :1], dtype=torch.bool)
        x = x + tie * (1.0 - 2.0 * (torch.arange(C) % 2)).view(1, C, 1, 1)
        assert C == 1 or float(x.to(dt).float().std(dim=1, unbiased=False).min()) >= 0.4
    else:   # ill-conditioned: a large common offset, and pixel 0 of image 0 with all channels equal (variance 0)
        x = ILL_OFFSET + 0.5 * torch.randn(shape, generator=_gen(seed))
        x[0, :, 0, 0] = 0.75
    s = SimpleNamespace(B=B, C=C, N=N, d=d, dt=dt, wb=wb, kind="WithBias" if wb else "BiasFree")
    s.x = x.to(dt)
    s.w = 1.0 + 0.2 * torch.randn(C, generator=_gen(seed + 1))
    s.b = 0.1 * torch.randn(C, generator=_gen(seed + 2)) if wb else None
    s.dy = torch.randint(-3, 4, shape, generator=_gen(seed + 3)).float().to(dt)
    s.dres = torch.randn(shape, generator=_gen(seed + 4)).to(dt)
    assert B * N * 3 < 2 ** 24
    return s


def reference(s, prec=torch.float64):
    """The oracle and its autograd at precision `prec` on the inputs as stored."""
    x = s.x.to(prec).clone().requires_grad_(True)
    w = s.w.to(prec).clone().requires_grad_(True)
    b = s.b.to(prec).clone().requires_grad_(True) if s.wb else None
    y = R.layernorm_nchw(x, w, b, s.kind)
    y.backward(s.dy.to(prec))
    return SimpleNamespace(y=y.detach(), dx_ln=x.grad, dw=w.grad, db=b.grad if s.wb else None)


@functools.lru_cache(maxsize=6)
def case(B, C, N, d, wb, data="plain"):
    s = make_inputs(B, C, N, d, wb, data)
    r = reference(s)
    xd = s.x.double()
    mu = xd.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(dim=1, keepdim=True) + R.LN_EPS)
    xhat = (xd - mu) * rstd if wb else xd * rstd
    s.y, s.dx_ln, s.dw = r.y, r.dx_ln, r.dw
    s.dx = r.dx_ln + s.dres.double()
    s.S = (s.dy.double() * xhat).abs().sum(dim=(0, 2, 3))
    s.db = s.dy.double().sum(dim=(0, 2, 3)).float()          # integers: exact
    s.mean, s.rstd = mu.reshape(B, N), rstd.reshape(B, N)
    return s


def dgamma_bound(B, N):
    return 4 * next(m for upto, m in DGAMMA_ORACLE_F32 if B * N <= upto)


def measure_fp32_oracle(cases, data="plain"):
    """Worst normalised dgamma error of the oracle evaluated in fp32 on the CPU (where DGAMMA_ORACLE_F32* come from)."""
    worst = 0.0
    for B, C, N, d, wb in sorted(set(cases)):
        s = case(B, C, N, d, wb, data)
        e = (reference(s, torch.float32).dw.double() - s.dw).abs() / s.S.clamp_min(1e-300)
        worst = max(worst, float(e[s.S > 0].max()) if bool((s.S > 0).any()) else 0.0)
    return worst


# --------------------------------------------------------------------------- assertions
def assert_elementwise(got, ref, dt, what, scale=None):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    tol = FLOOR * (ref.abs().max() if scale is None else scale) + (BF16_UNIT * ref.abs() if dt == BF16 else 0.0)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int((err - tol).nan_to_num(nan=float("inf")).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at flat index {i}: "
                             f"got {float(got[i])!r}, ref {float(ref[i])!r}, allowed {float(tol[i] if tol.dim() else tol):.3e}")


def assert_stats(mean, rstd, s, what):
    for name, got, ref, scale in (("mean", mean, s.mean, s.x.double().abs().max()), ("rstd", rstd, s.rstd, s.rstd.abs().max())):
        err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
        assert bool((err <= FLOOR * scale).all()), f"{what}: {name} off by {float(err.max()):.3e} (allowed {float(FLOOR * scale):.3e})"


def assert_dgamma(dw, s, what, prior=None, times=1, bound=None):
    bound = dgamma_bound(s.B, s.N) if bound is None else bound
    ref = times * s.dw + (prior.double() if prior is not None else 0.0)
    tol = times * bound * s.S + (times * F32_ADD * ref.abs() if prior is not None else 0.0)
    err = (dw.detach().cpu().double() - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        c = int((err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).argmax())
        raise AssertionError(f"{what}: dgamma of {int(bad.sum())} channels outside the bound; worst channel {c}: error "
                             f"{float(err[c]):.3e} = {float(err[c] / s.S[c].clamp_min(1e-300)):.3e} S_c, allowed {float(tol[c]):.3e}")


def assert_dbeta(db, s, what, prior=None, times=1):
    ref = times * s.db + (prior if prior is not None else 0.0)
    got = db.detach().cpu()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero().flatten().tolist()
        raise AssertionError(f"{what}: dbeta is not the exact integer sum at channels {bad[:8]} ({len(bad)} in all): "
                             f"got {got[bad[:8]].tolist()}, want {ref[bad[:8]].tolist()}")


def run_fwd(s, want_stats=True, x=None):
    o = ops()
    return o.ln_fwd(s.x.to(DEV) if x is None else x, s.w.to(DEV), s.b.to(DEV) if s.wb else None, s.wb, want_stats)


def run_bwd(s, mean, rstd, dres=True, grads=None, x=None, dy=None, dr=None):
    """grads = (dw, db) to accumulate into; None: fresh NaN-filled buffers that the call must overwrite."""
    o = ops()
    acc = grads is not None
    dw = grads[0] if acc else torch.full((s.C,), float("nan"), device=DEV)
    db = (grads[1] if acc else torch.full((s.C,), float("nan"), device=DEV)) if s.wb else None
    dres_t = (s.dres.to(DEV) if dr is None else dr) if dres else None
    dx = o.ln_bwd(s.dy.to(DEV) if dy is None else dy, s.x.to(DEV) if x is None else x, s.w.to(DEV), mean, rstd, dres_t, s.wb,
                  dw, db, acc)
    return dx, dw, db


def check_all(s, what, dg_bound=None):
    """Forward and backward of one case against its reference, every output."""
    y, mean, rstd = run_fwd(s)
    assert_elementwise(y, s.y, s.dt, f"{what}: y")
    assert_stats(mean, rstd, s, what)
    dx, dw, db = run_bwd(s, mean, rstd)
    assert_elementwise(dx, s.dx, s.dt, f"{what}: dx")
    assert_dgamma(dw, s, what, bound=dg_bound)
    if s.wb:
        assert_dbeta(db, s, what)


def assert_plans_fit(pl, C, what):
    for p in pl:
        assert capacity(p) >= C, f"{what}: the plan {p} does not hold {C} channels"


# --------------------------------------------------------------------------- the sweeps
def _sweep(monkeypatch, c, why):
    B, C, N, d, wb, form = c
    todo = resolve_form(monkeypatch, B, C, N, d, form)
    if not todo:
        pytest.skip(why)

    def one(f, pf, pb):
        assert_plans_fit((pf, pb), C, case_id(c))
        if d == "bf16" and N % 2:
            assert pf["vec"] == 1 and pb["vec"] == 1 and pf["family"] == pb["family"] == "block", (pf, pb)
        for p in (pf, pb):
            assert p["gx"] * p["tiles"] * 64 * p["vec"] >= N, p
        check_all(case(B, C, N, d, wb), f"{case_id(c)} MI_LN_FORM={f} fwd {pf} bwd {pb}")
    run_forms(monkeypatch, todo, one)


@pytest.mark.parametrize("c", CHANNEL_CASES, ids=case_id)
def test_channel_sweep(monkeypatch, c):
    """Every channel bin at its first, last and first-past-the-last count, in every form."""
    _sweep(monkeypatch, c, f"no other family at C={c[1]} N={c[2]} {c[3]}")


@pytest.mark.parametrize("c", PIXEL_CASES, ids=case_id)
def test_pixel_sweep(monkeypatch, c):
    """Pixel counts around one, two and four tiles and around a workgroup's tiles, three images; odd N in bf16 takes the
    one-pixel fallback."""
    _sweep(monkeypatch, c, f"no other family at C={c[1]} N={c[2]} {c[3]}")


@pytest.mark.parametrize("direction,C,form,ws", [("bwd", 49, "default", 4), ("bwd", 97, "default", 8), ("bwd", 193, "default", 16),
                                                   ("fwd", 97, "default", 2), ("fwd", 193, "wave", 4), ("fwd", 384, "wave", 4)])
@pytest.mark.parametrize("d", ["f32", "bf16"])
def test_waves_with_an_empty_or_partial_channel_slice(monkeypatch, d, direction, C, form, ws):
    """Wave-owned kernels whose last slices hold one channel or none (backward C = 49: 24 + 24 + 1 + 0), and the forward
    with four waves per tile, which only MI_LN_FORM=wave reaches."""
    B, N = 3, 130
    set_form(monkeypatch, form)
    pl = plans(B, C, N, d)
    p = pl[0] if direction == "fwd" else pl[1]
    assert p["family"] == "wave" and p["WS"] == ws, p
    assert C == 384 or p["CB"] * (p["WS"] - 1) >= C or C - p["CB"] * (p["WS"] - 1) == 1, p
    check_all(case(B, C, N, d, True), f"C{C} {direction} {p}")


@pytest.mark.parametrize("c", MISALIGNED, ids=lambda c: f"C{c[1]}-{c[3]}")
def test_misaligned_bf16_operand_takes_the_one_pixel_form(monkeypatch, c):
    B, C, N, op = c
    set_form(monkeypatch, "default")
    s = case(B, C, N, "bf16", True)
    pf, pb = plans(B, C, N, "bf16", aligned=False)
    assert pf["vec"] == 1 and pb["vec"] == 1 and pf["family"] == pb["family"] == "block", (pf, pb)
    assert plans(B, C, N, "bf16")[0]["vec"] == 2, "the aligned call should move two pixels per lane"

    def odd(t):
        buf = torch.zeros(t.numel() + 3, dtype=t.dtype, device=DEV)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 4 == 2 and v.is_contiguous()
        return v
    if op == "x_fwd":
        y, mean, rstd = run_fwd(s, x=odd(s.x))
        assert_elementwise(y, s.y, s.dt, f"{c}: y")
        assert_stats(mean, rstd, s, str(c))
        return
    _, mean, rstd = run_fwd(s)
    kw = {"dy": {"dy": odd(s.dy)}, "x": {"x": odd(s.x)}, "dres": {"dr": odd(s.dres)}}[op]
    dx, dw, db = run_bwd(s, mean, rstd, **kw)
    assert_elementwise(dx, s.dx, s.dt, f"{c}: dx")
    assert_dgamma(dw, s, str(c))
    assert_dbeta(db, s, str(c))


@pytest.mark.parametrize("form", ["default", "block"])
@pytest.mark.parametrize("c", TWO_STAGE, ids=lambda c: f"B{c[0]}-C{c[1]}-N{c[2]}-{'two' if c[3] else 'one'}stage")
def test_row_reduction_stages(monkeypatch, c, form):
    """132 partial rows take reduce_rows_kernel twice, 128 once; the last tile of every image holds one pixel."""
    B, C, N, two = c
    set_form(monkeypatch, form)
    pb = plans(B, C, N, "f32")[1]
    assert pb["family"] == ("wave" if form == "default" else "block"), pb
    assert pb["rows"] == (132 if two else 128) and pb["two_stage"] == two, pb
    check_all(case(B, C, N, "f32", True), f"{c} {pb}")


# --------------------------------------------------------------------------- options
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d,C,N", [("f32", 48, 65), ("bf16", 96, 130), ("bf16", 193, 130), ("f32", 385, 65)])
def test_without_residual_and_without_statistics(monkeypatch, d, C, N, form):
    """dres = NULL leaves dx the LayerNorm gradient alone; mean = rstd = NULL leaves y bit for bit what it is with them."""
    B = 2
    todo = resolve_form(monkeypatch, B, C, N, d, form)
    if not todo:
        pytest.skip(f"MI_LN_FORM={form} changes nothing at C={C}")
    set_form(monkeypatch, todo[0][0])
    pl = todo[0][1:]
    for wb in (True, False):
        s = case(B, C, N, d, wb)
        y, mean, rstd = run_fwd(s)
        y0, m0, r0 = run_fwd(s, want_stats=False)
        assert m0 is None and r0 is None and torch.equal(y, y0), f"{pl[0]}: y changes with the statistics outputs"
        dx, dw, db = run_bwd(s, mean, rstd, dres=False)
        assert_elementwise(dx, s.dx_ln, s.dt, f"{pl[1]} wb={wb}: dx without dres")
        assert_dgamma(dw, s, f"{pl[1]} wb={wb}")
        if wb:
            assert_dbeta(db, s, f"{pl[1]}")


def _priors(C, seed):
    dw0 = torch.randn(C, generator=_gen(seed)) * 3.0
    db0 = torch.randint(-5, 6, (C,), generator=_gen(seed + 1)).float()
    return dw0, db0


@pytest.mark.parametrize("form", ["default", "block"])
@pytest.mark.parametrize("d,B,C,N", [("f32", 3, 48, 65), ("bf16", 2, 192, 130), ("f32", 3, 16, 2753), ("bf16", 2, 768, 65)])
def test_accumulate_adds_to_what_is_there(monkeypatch, d, B, C, N, form):
    """accumulate onto random non-zero dw / db (integer db): the result is prior + gradient, not 2 x gradient or the
    gradient alone."""
    set_form(monkeypatch, form)
    for wb in (True, False):
        s = case(B, C, N, d, wb)
        _, mean, rstd = run_fwd(s)
        dw0, db0 = _priors(C, 7 * C + N)
        dx, dw, db = run_bwd(s, mean, rstd, grads=(dw0.to(DEV), db0.to(DEV)))
        what = f"{form} {d} B{B} C{C} N{N} wb={wb}"
        assert_elementwise(dx, s.dx, s.dt, what + ": dx")
        assert_dgamma(dw, s, what, prior=dw0)
        if wb:
            assert_dbeta(db, s, what, prior=db0)


@pytest.mark.parametrize("d,B,C,N,form", [("bf16", 3, 48, 130, "default"), ("f32", 3, 192, 2753, "block")])
def test_deferred_window_sums_both_calls(monkeypatch, d, B, C, N, form):
    """Two accumulating backward calls inside a deferred window: nothing lands before the flush, prior + 2 x gradient
    after it (deferred_reduce_kernel, two generations because both jobs write the same gradient)."""
    set_form(monkeypatch, form)
    o = ops()
    s = case(B, C, N, d, True)
    _, mean, rstd = run_fwd(s)
    dw0, db0 = _priors(C, 11 * C + N)
    dw, db = dw0.to(DEV), db0.to(DEV)
    tok = o.deferred_begin(4 * lib().lib().mi_ln_bwd_workspace(B, C, N) + (8 << 20), torch.device(DEV))
    assert tok is not None
    try:
        o.deferred_record(True)
        for _ in range(2):
            dx, _, _ = run_bwd(s, mean, rstd, grads=(dw, db))
            assert_elementwise(dx, s.dx, s.dt, "dx inside the window")
        assert o.deferred_pending() == 2
        torch.cuda.synchronize()
        assert torch.equal(dw.cpu(), dw0) and torch.equal(db.cpu(), db0), "a deferred sum landed before the flush"
        o.deferred_flush()
        assert o.deferred_pending() == 0
    finally:
        o.deferred_end(tok)
    assert_dgamma(dw, s, "deferred", prior=dw0, times=2)
    assert_dbeta(db, s, "deferred", prior=db0, times=2)


# --------------------------------------------------------------------------- ill-conditioned data
def _variance_formulas_fp32(s):
    """The oracle's two-pass formula and the one-pass E[x^2] - mu^2, both in fp32 on the CPU: worst error of y over the
    allowed error (> 1: outside the fp32 bound)."""
    x = s.x.float()
    w = s.w.view(1, -1, 1, 1)
    b = s.b.view(1, -1, 1, 1) if s.wb else 0.0
    mu = x.mean(dim=1, keepdim=True)
    out = []
    for var in (((x - mu) ** 2).mean(dim=1, keepdim=True), (x * x).mean(dim=1, keepdim=True) - mu * mu):
        rs = 1.0 / torch.sqrt(var.clamp_min(0.0) + R.LN_EPS)
        y = (x - mu) * rs * w + b if s.wb else x * rs * w
        out.append(float(((y.double() - s.y).abs() / (FLOOR * _ill_scale(s.y))).max()))
    return out


def _ill_scale(ref):
    """max |ref| over the ordinary pixels: the constant pixel (rstd = 1 / sqrt(eps) = 316) must not set the scale."""
    r = ref.clone()
    r[0, :, 0, 0] = 0.0
    return r.abs().max()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C", [48, 192])
@pytest.mark.parametrize("wb", [True, False], ids=["bias", "nobias"])
def test_ill_conditioned_needs_the_two_pass_variance(monkeypatch, wb, C, form):
    """fp32, x = 50 + 0.5 randn: |mean| is 100 standard deviations, so E[x^2] - mu^2 loses the variance to cancellation.
    Offset 50 is the issue's value and did not need widening.  Errors of y in units of the fp32 bound (2e-5 of max |y|
    over the ordinary pixels), evaluated in fp32 on the CPU: two-pass 0.27 (C = 48 bias), 0.008 (C = 48 no bias), 0.24
    (C = 192 bias), 0.010 (C = 192 no bias); one-pass 66, 104, 73, 72.  The test re-checks both before it relies on them.
    Pixel 0 of image 0 has every channel at 0.75: variance 0, rstd = 1 / sqrt(eps).  It is held to the bound as stated (of
    the whole tensor's maximum); the other pixels are held to their own maximum, so that its rstd of 316 and its dx of
    about 1000 do not set the scale of their bound."""
    B, N = 2, 130
    s = case(B, C, N, "f32", wb, "ill")
    two, one = _variance_formulas_fp32(s)
    assert two <= 1.0 < one, f"CPU fp32: two-pass {two:.2f}, one-pass {one:.2f} of the bound - the data do not separate them"
    todo = resolve_form(monkeypatch, B, C, N, "f32", form)
    if not todo:
        pytest.skip(f"MI_LN_FORM={form} changes nothing at C={C}")
    set_form(monkeypatch, todo[0][0])
    what = f"ill C{C} wb={wb} {form}"
    y, mean, rstd = run_fwd(s)
    dx, dw, db = run_bwd(s, mean, rstd)
    assert float(s.rstd[0, 0]) == pytest.approx(R.LN_EPS ** -0.5, rel=1e-12)
    assert_stats(mean, rstd, s, what)
    rest_rstd = s.rstd.clone()
    rest_rstd[0, 0] = 0.0
    err = (rstd.cpu().double() - s.rstd).abs()
    err[0, 0] = 0.0
    assert bool((err <= FLOOR * rest_rstd.max()).all()), f"{what}: rstd of the ordinary pixels off by {float(err.max()):.3e}"
    for name, got, ref in (("y", y, s.y), ("dx", dx, s.dx)):
        got = got.cpu().double()
        assert_elementwise(got[0, :, 0, 0], ref[0, :, 0, 0], F32, f"{what}: {name} of the constant pixel", scale=ref.abs().max())
        got, ref = got.clone(), ref.clone()
        got[0, :, 0, 0] = 0.0
        ref[0, :, 0, 0] = 0.0
        assert_elementwise(got, ref, F32, f"{what}: {name} of the ordinary pixels")
    assert_dgamma(dw, s, what, bound=DGAMMA_BOUND_ILL)
    if wb:
        assert_dbeta(db, s, what)


# --------------------------------------------------------------------------- guard words (C ABI)
GUARD = 256     # elements on each side
GUARD_CASES = [("f32", 3, 49, 65, "wave"), ("bf16", 3, 49, 130, "wave"), ("bf16", 3, 193, 130, "wave"), ("f32", 2, 193, 65, "wave"),
               ("f32", 3, 49, 65, "block"), ("bf16", 3, 17, 130, "block"), ("f32", 2, 385, 65, "default"),
               ("bf16", 3, 16, 129, "default"), ("f32", 3, 16, 2753, "default"), ("f32", 3, 16, 2753, "block")]


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill):
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return bool((g == fill).all())


@pytest.mark.parametrize("c", GUARD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_outputs_and_workspace_stay_inside_their_buffers(monkeypatch, c):
    """y, dx, mean, rstd, dw, db and a workspace of exactly mi_ln_bwd_workspace bytes, each carved out of a sentinel-filled
    buffer: the sentinels on both sides are untouched, at the ragged-N and empty-slice cases of both families, and the
    rows the plan says are written (plus the two-stage scratch) fit the workspace formula."""
    d, B, C, N, form = c
    set_form(monkeypatch, form)
    o, L = ops(), lib()
    pf, pb = plans(B, C, N, d)
    if form != "default":
        assert form in (pf["family"], pb["family"]), (pf, pb)
    s = case(B, C, N, d, True)
    n = B * C * N
    ws_bytes = L.lib().mi_ln_bwd_workspace(B, C, N)
    assert ws_bytes % 4 == 0 and (pb["rows"] + (32 if pb["two_stage"] else 0)) * 2 * C * 4 <= ws_bytes, (pb, ws_bytes)
    act, par = -7.0, 12345.0
    ybuf, y = _guarded(n, s.dt, act)
    dxbuf, dx = _guarded(n, s.dt, act)
    mbuf, mean = _guarded(B * N, F32, par)
    rbuf, rstd = _guarded(B * N, F32, par)
    dwbuf, dw = _guarded(C, F32, par)
    dbbuf, db = _guarded(C, F32, par)
    wsbuf, ws = _guarded(ws_bytes // 4, F32, par)
    assert all(t.data_ptr() % 256 == 0 for t in (y, dx, mean, rstd, dw, db, ws))
    x, w, b, dy, dres = (t.to(DEV) for t in (s.x, s.w, s.b, s.dy, s.dres))
    dtc = o._dt(x)
    L.check(L.lib().mi_ln_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, C, N,
                              1, dtc, o._stream()), "ln_fwd")
    L.check(L.lib().mi_ln_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dres.data_ptr(),
                              dx.data_ptr(), dw.data_ptr(), db.data_ptr(), B, C, N, 1, 0, dtc, ws.data_ptr(), o._stream()), "ln_bwd")
    torch.cuda.synchronize()
    for name, buf, m, fill in (("y", ybuf, n, act), ("dx", dxbuf, n, act), ("mean", mbuf, B * N, par), ("rstd", rbuf, B * N, par),
                               ("dw", dwbuf, C, par), ("db", dbbuf, C, par), ("workspace", wsbuf, ws_bytes // 4, par)):
        assert _guards_intact(buf, m, fill), f"{c}: a guard word next to {name} was overwritten ({pf} / {pb})"
    shape = (B, C, 1, N)
    assert_elementwise(y.view(shape), s.y, s.dt, f"{c}: y")
    assert_elementwise(dx.view(shape), s.dx, s.dt, f"{c}: dx")
    assert_stats(mean, rstd, s, str(c))
    assert_dgamma(dw, s, str(c))
    assert_dbeta(db, s, str(c))

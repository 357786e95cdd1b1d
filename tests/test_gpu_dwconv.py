"""Depthwise convolutions (csrc/dwconv.hip, csrc/dwstream.hip) across every launch plan and seam, against a plain fp64 CPU
reference (F.conv2d(groups=C) and its autograd; gelu(y1) * y2 for the GDFN gate).

Each case names the plan it is meant to reach and asserts it with mi_dwconv_plan, so a retune of pick_band / dw_tiling
shows up as a failing case instead of a silent loss of coverage; test_*_matrix_is_covered check the tables as a whole.

Data are small integers wherever the operation allows it (inputs in [-3, 3], taps and biases multiples of 1/2, dy / dg in
[-3, 3]): forward, dx, dW and db are then exact in fp32 and forward and dx also in bf16, whatever the summation order, and
are compared bitwise.  The gate outputs and the gate backward carry GELU and are held to tolerances.  Cases with tens of
thousands of planes (the tall bands) are generated on the device and checked on a subset of channels: depthwise channels
are independent, and dW / db of a channel only sum over that channel's images."""
import math

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTS = {"f32": F32, "bf16": BF16}
TOL = {F32: 2e-5, BF16: 2.5e-2}     # gate outputs / gate backward, of max |ref| (tests/test_gpu_primitives.py)
GELU_BF16_ABS = 3.0e-4              # |refitted GELU - erf GELU| (common.h; test_gpu_round4.py checks the formula)

ENTRIES = ("fwd", "fwd_nob", "gate_fwd", "gate_fwd_noy", "bwd", "bwd_dw", "bwd_dx", "gate_bwd", "gate_bwd_nodw",
           "rc", "rc_nob", "rc_nodw", "rc_nob_nodw")
PLAN_OP = {"fwd": "fwd", "fwd_nob": "fwd", "gate_fwd": "gate_fwd", "gate_fwd_noy": "gate_fwd", "bwd": "bwd",
           "bwd_dw": "bwd", "bwd_dx": "bwd", "gate_bwd": "gate_bwd", "gate_bwd_nodw": "gate_bwd", "rc": "gate_bwd",
           "rc_nob": "gate_bwd", "rc_nodw": "gate_bwd", "rc_nob_nodw": "gate_bwd"}
GATE = {e for e in ENTRIES if PLAN_OP[e] in ("gate_fwd", "gate_bwd")}
CORE = ("fwd", "bwd", "gate_bwd")   # run in both dtypes at every plan point; the other entries alternate dtypes


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def ops():
    from image_restoration_amd import ops as o
    return o


def lib():
    from image_restoration_amd import _lib
    return _lib.lib()


def plan(B, C, H, W, ks, entry):
    return ops().dwconv_plan(B, C, H, W, ks, PLAN_OP[entry])


def seam(H, band):
    """Which seam of the band grid a plane height sits on."""
    if H in (1, 2):
        return str(H)
    if H < band:
        return "lt"
    return {0: "kb", 1: "kb+1", band - 1: "kb+b-1"}.get(H % band, "other")


# --------------------------------------------------------------------------- case tables
# Register-streaming rows: (W, H, B, C, band, uni).  C is the plain entries' channel count; the gate entries run on 2C
# channels, i.e. on the same B*C planes, so both reach the same plan.  Band 8 takes a handful of planes; the tall bands
# need planes * ceil(H / band) / (64 / (W / 4)) >= 8192 (one more channel than the minimum leaves the last workgroup
# partly inactive).  H = 8 * G puts nb at a multiple of the lane groups per wave: the UNI form.
STREAM = [(W, H, 2, 3, 8, None) for W in (16, 32, 64, 128, 256)
          for H in sorted({1, 2, 5, 16, 17, 23, 8 * (256 // W)})] + [
    (16, 32, 4, 16385, 16, False),
    (32, 17, 2, 16385, 16, False),
    (64, 31, 1, 16385, 16, False),
    (128, 32, 1, 8193, 16, True),
    (256, 17, 1, 4097, 16, True),
    (16, 64, 4, 16385, 32, False),
    (32, 33, 2, 16385, 32, False),
    (64, 63, 1, 16385, 32, False),
    (128, 64, 1, 8193, 32, True),
    (256, 33, 1, 4097, 32, True),
    (16, 40, 8, 16385, 64, False),
    (16, 1, 8, 16385, 64, False),
    (32, 64, 4, 16385, 64, False),
    (32, 2, 4, 16385, 64, False),
    (64, 65, 1, 16385, 64, False),
    (128, 127, 1, 8193, 64, True),
    (256, 40, 1, 8193, 64, True),
]


def _stream_uni(W, H, band):
    G = 256 // W
    return G == 1 or math.ceil(H / band) % G == 0


def _row_id(W, H, B, C, band):
    G = 256 // W
    nb = math.ceil(H / band)
    tail = "-tail" if (B * C * nb) % (4 * G) else ""
    return f"W{W}-H{H}-band{band}-{seam(H, band)}-{'uni' if _stream_uni(W, H, band) else 'nonuni'}{tail}"


def _entries_for(i):
    """(entry, dtype, data) of plan row i: CORE in both dtypes, every other entry once, one random fp32 set."""
    out = [(e, d, "int") for e in CORE for d in ("f32", "bf16")]
    out += [(e, ("f32", "bf16")[(i + k) % 2], "int") for k, e in enumerate(ENTRIES) if e not in CORE]
    out += [(e, "f32", "rand") for e in CORE]
    return out


STREAM_CASES = [pytest.param(r, e, d, dat, id=f"{_row_id(*r[:5])}-{e}-{d}-{dat}")
                for i, r in enumerate(STREAM) for e, d, dat in _entries_for(i)]


# LDS-tiled rows: (W, H, ks, group).  The tile width follows W (16 below 24, 32 below 48, else 64), a tile is
# 256 / (tw / 4) = tyn rows per row-of-threads, and 3x3 planes of >= 2 tyn rows take 4 (plain) or 2 (gate) rows per thread.
# H sits at th - 1, th and th + 1 of every tile height; W walks every width of its tile width (ragged tiles_x, W % 4 != 0,
# a multiple of 4 that is no power of two).
LDS_W = {16: (5, 13, 17), 32: (24, 31, 47), 64: (48, 70, 96, 130)}


def _lds_rows():
    rows = []
    for tw, ws in LDS_W.items():
        tyn = 256 // (tw // 4)
        hs = {("plain", 3): [tyn - 1, tyn, tyn + 1, 4 * tyn - 1, 4 * tyn, 4 * tyn + 1],
              ("gate", 3): [tyn - 1, tyn, tyn + 1, 2 * tyn - 1, 2 * tyn, 2 * tyn + 1]}
        for ks in (5, 7):
            hs[("plain", ks)] = hs[("gate", ks)] = [tyn - 1, tyn, tyn + 1]
        k = 0
        for (group, ks), hl in hs.items():
            for H in hl:
                rows.append((ws[k % len(ws)], H, ks, group))
                k += 1
    return rows


LDS = _lds_rows()


def _lds_entries(group, i):
    core = ("fwd", "bwd") if group == "plain" else ("gate_bwd",)
    rest = ("fwd_nob", "bwd_dw", "bwd_dx") if group == "plain" else ("gate_fwd", "gate_fwd_noy", "gate_bwd_nodw")
    out = [(e, d, "int") for e in core for d in ("f32", "bf16")]
    out += [(e, ("f32", "bf16")[(i + k) % 2], "int") for k, e in enumerate(rest)]
    out += [(e, "f32", "rand") for e in core]
    return out


def _lds_id(W, H, ks, group):
    return f"W{W}-H{H}-k{ks}-{group}"


LDS_CASES = [pytest.param(r, e, d, dat, id=f"{_lds_id(*r)}-{e}-{d}-{dat}")
             for i, r in enumerate(LDS) for e, d, dat in _lds_entries(r[3], i)]


# --------------------------------------------------------------------------- data, memory layouts, the runner
def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _data(shape, dtype, seed, rand, lo=-3, hi=3):
    if rand:
        return torch.randn(shape, generator=_gen(seed), device=DEV, dtype=F32).to(dtype)
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed), device=DEV, dtype=torch.int8).to(dtype)


def _taps(C, ks, seed, rand):
    """[C, ks*ks] fp32: multiples of 1/2 in [-1, 1] (7x7: integers in [-1, 1]) - every sum stays exact in bf16."""
    if rand:
        return torch.randn((C, ks * ks), generator=_gen(seed), device=DEV) / ks
    q = 1 if ks == 7 else 2
    return torch.randint(-q, q + 1, (C, ks * ks), generator=_gen(seed), device=DEV).float() / q


def _bias(C, ks, seed, rand):
    if rand:
        return 0.1 * torch.randn((C,), generator=_gen(seed), device=DEV)
    q = 1 if ks == 7 else 2
    return torch.randint(-q, q + 1, (C,), generator=_gen(seed), device=DEV).float() / q


def _nbytes(shape, dtype):
    return math.prod(shape) * torch.empty((), dtype=dtype).element_size()


class Mem:
    """Plain device tensors."""

    def put(self, t):
        return t

    def out(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=DEV)

    def ws(self, nbytes):
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)

    def check(self):
        pass


GUARD16 = -91      # 0xffa5: a NaN in bf16, and two of them a NaN in fp32


class Guarded(Mem):
    """Inputs sit between margins of 0xff bytes (a NaN in fp32 and bf16): a row read from outside its plane poisons the
    result, even times a zero tap.  Outputs and the workspace (contents 0xff) sit between guards of 0xffa5 words (another
    NaN) that must come back bitwise unchanged; a store of anything computed from the 0xff margins cannot pass for them."""

    def __init__(self, guard):
        self.guard = max(4096, -(-guard // 4096) * 4096)
        self.slots = []

    def _slot(self, nbytes, guarded=True):
        g = self.guard
        buf = torch.full((g + nbytes + g,), 255, dtype=torch.uint8, device=DEV)
        if guarded:
            buf[:g].view(torch.int16).fill_(GUARD16)
            buf[g + nbytes:].view(torch.int16).fill_(GUARD16)
            self.slots.append((buf, g, g + nbytes))
        return buf[g:g + nbytes]

    def put(self, t):
        v = self._slot(t.numel() * t.element_size(), guarded=False).view(t.dtype).view(t.shape)
        v.copy_(t)
        return v

    def out(self, shape, dtype):
        return self._slot(_nbytes(shape, dtype)).view(dtype).view(shape)

    def ws(self, nbytes):
        return self._slot(nbytes)          # exactly mi_dwconv_bwd_workspace bytes, NaN-filled

    def check(self):
        torch.cuda.synchronize()
        for k, (buf, lo, hi) in enumerate(self.slots):
            below = int((buf[:lo].view(torch.int16) != GUARD16).sum())
            past = int((buf[hi:].view(torch.int16) != GUARD16).sum())
            assert below == 0 and past == 0, f"buffer {k}: {below} words written below it, {past} past its end"


class Offset(Mem):
    """Every activation starts one element past a 16-byte boundary: vec_ok is false, the scalar paths run."""

    def _flat(self, n, dtype):
        return torch.empty(n + 1, dtype=dtype, device=DEV)[1:]

    def put(self, t):
        v = self._flat(t.numel(), t.dtype).view(t.shape)
        v.copy_(t)
        return v

    def out(self, shape, dtype):
        return self._flat(math.prod(shape), dtype).view(shape)


def _p(t):
    return None if t is None else t.data_ptr()


def _ok(rc, what):
    assert rc == 0, f"{what}: rc={rc}: {lib().mi_last_error().decode()}"


def _pick(n, nb, G, planes_per_image, images):
    """Channels checked against the reference: all of them when few, else the first and last, both sides of the first
    workgroup boundaries and of the last workgroup's start (4 G units per workgroup), and a stride through the rest."""
    if n <= 40:
        return list(range(n))
    per_wg = 4 * G
    total = planes_per_image * images
    s = {0, 1, n - 2, n - 1}
    for unit in (per_wg, 2 * per_wg, 7 * per_wg, (total * nb - 1) // per_wg * per_wg):
        p = unit // nb
        for q in (p - 1, p, p + 1):
            if 0 <= q < total:
                s.add(q % planes_per_image)
    s.update(range(3, n, max(1, n // 16)))
    return sorted(c for c in s if 0 <= c < n)


def _sub(t, idx):
    return t.index_select(1, torch.tensor(idx, device=t.device)).cpu().double()


def _exact(got, ref, what):
    got = got.detach().cpu().double()
    nbad = int((got != ref).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} values differ, max |diff| " \
                      f"{float((got - ref).abs().nan_to_num(float('inf')).max())}"


def _near(got, ref, tol, what):
    got = got.detach().cpu().double()
    err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    assert err < tol, f"{what}: rel err {err:.3e} >= {tol:.1e}"


def _check(got, ref, dtype, exact, what):
    if exact:
        _exact(got, ref, what)
    else:
        _near(got, ref, TOL[dtype], what)


def _gate_fwd_check(g, y1, y2, dtype, what):
    """g = gelu(y1) * y2, with y the values the kernel gated (fp64).  bf16: the refitted GELU's stated bound times |y2| plus
    half a bf16 step of the result; fp32: the erf form, 2e-5 of max |ref|."""
    ref = F.gelu(y1) * y2
    got = g.detach().cpu().double()
    if dtype == F32:
        _near(got, ref, TOL[F32], what)
        return
    slack = GELU_BF16_ABS * y2.abs()
    bound = slack + 2.0 ** -8 * (ref.abs() + slack) + 1e-30
    nover = int(((got - ref).abs() > bound).sum() + got.isnan().sum())
    assert nover == 0, f"{what}: {nover} values beyond the bf16 GELU bound"


def run(entry, dtype, B, C, H, W, ks=3, rand=False, mem=None, seed=0, acc_prefill=None):
    """Runs one entry point through the C-ABI on (B, C, H, W) and checks the channels of _pick against fp64.  C counts the
    entry's conv channels (2h for the gate entries).  acc_prefill: (dW, db) the call accumulates into (accumulate = 1)."""
    mem = mem or Mem()
    L, o = lib(), ops()
    dt = 0 if dtype == F32 else 1
    st = o._stream()
    gate = entry in GATE
    exact = not rand
    P = ks // 2
    n_sel = C // 2 if gate else C
    pl = plan(B, C, H, W, ks, entry)
    nb = pl["nb"] if pl["family"] == "stream" else pl["bands"]
    G = 64 // pl["lpr"] if pl["family"] == "stream" else 1
    sel = _pick(n_sel, nb, G, n_sel, B)
    idx = sel + [j + C // 2 for j in sel] if gate else sel
    w = _taps(C, ks, seed + 1, rand)
    wr = w[idx].cpu().double().view(len(idx), 1, ks, ks)
    with_bias = "nob" not in entry and entry != "gate_fwd_noy"
    bias = _bias(C, ks, seed + 2, rand) if with_bias else None
    br = bias[idx].cpu().double() if bias is not None else None
    x = mem.put(_data((B, C, H, W), dtype, seed, rand))
    conv = lambda t, wt, bt: F.conv2d(t, wt, bt, padding=P, groups=wt.shape[0])   # noqa: E731
    accumulate = 1 if acc_prefill is not None else 0
    want_dw = entry in ("bwd", "bwd_dw", "gate_bwd", "rc", "rc_nob")
    ws = mem.ws(L.mi_dwconv_bwd_workspace(B, C, H, W, ks)) if PLAN_OP[entry] in ("bwd", "gate_bwd") else None
    dw = db = None
    if want_dw:
        if acc_prefill is not None:
            dw, db = mem.put(acc_prefill[0].clone()), mem.put(acc_prefill[1].clone())
        else:
            dw, db = mem.out((C, ks * ks), F32), mem.out((C,), F32)

    if PLAN_OP[entry] == "fwd":
        y = mem.out((B, C, H, W), dtype)
        _ok(L.mi_dwconv_fwd(_p(x), _p(w), _p(bias), _p(y), B, C, H, W, ks, dt, st), entry)
        mem.check()
        _check(y[:, idx], conv(_sub(x, idx), wr, br), dtype, exact, f"{entry} y")
        return pl
    if PLAN_OP[entry] == "gate_fwd":
        y = mem.out((B, C, H, W), dtype) if entry == "gate_fwd" else None
        g = mem.out((B, C // 2, H, W), dtype)
        _ok(L.mi_dwconv_gate_fwd(_p(x), _p(w), _p(bias), _p(y), _p(g), B, C, H, W, ks, dt, st), entry)
        mem.check()
        yr = conv(_sub(x, idx), wr, br)
        n = len(sel)
        if y is not None:
            _check(y[:, idx], yr, dtype, exact, "gate_fwd y")
            if rand:                        # the gate is evaluated on y as stored
                yr = _sub(y, idx)
        _gate_fwd_check(g[:, sel], yr[:, :n], yr[:, n:], dtype, f"{entry} g")
        return pl

    dx = None if entry in ("bwd_dw",) else mem.out((B, C, H, W), dtype)
    dpre = (acc_prefill[0][idx].cpu().double(), acc_prefill[1][idx].cpu().double()) if acc_prefill is not None else None
    xr = _sub(x, idx).requires_grad_(True)
    wrg = wr.clone().requires_grad_(True)
    if PLAN_OP[entry] == "bwd":
        dy = mem.put(_data((B, C, H, W), dtype, seed + 3, rand))
        _ok(L.mi_dwconv_bwd(_p(dy), None if entry == "bwd_dx" else _p(x), _p(w), _p(dx), _p(dw), _p(db),
                            B, C, H, W, ks, accumulate, dt, _p(ws), st), entry)
        mem.check()
        d = _sub(dy, idx)
        conv(xr, wrg, None).backward(d)
        gexact = exact
    else:
        n = len(sel)
        dg = mem.put(_data((B, C // 2, H, W), dtype, seed + 3, rand))
        dgr = _sub(dg, sel)
        if entry.startswith("gate_bwd"):
            y = mem.put(_data((B, C, H, W), dtype, seed + 4, rand))
            _ok(L.mi_dwconv_gate_bwd(_p(dg), _p(y), None if dw is None else _p(x), _p(w), _p(dx), _p(dw), _p(db),
                                     B, C, H, W, ks, accumulate, dt, _p(ws), st), entry)
            ys = _sub(y, idx).requires_grad_(True)
            (F.gelu(ys[:, :n]) * ys[:, n:]).backward(dgr)
            d = ys.grad
            conv(xr, wrg, None).backward(d)
        else:
            _ok(L.mi_dwconv_gate_bwd_recompute(_p(dg), _p(x), _p(w), _p(bias), _p(dx), _p(dw), _p(db),
                                               B, C, H, W, ks, accumulate, dt, _p(ws), st), entry)
            brg = br.clone().requires_grad_(True) if br is not None else None
            yr = conv(xr, wrg, brg)
            yr.retain_grad()
            (F.gelu(yr[:, :n]) * yr[:, n:]).backward(dgr)
            d = yr.grad
        mem.check()
        gexact = False
    if dx is not None:
        _check(dx[:, idx], xr.grad, dtype, gexact, f"{entry} dx")
    if dw is not None:
        rdw, rdb = wrg.grad.view(len(idx), ks * ks), d.sum(dim=(0, 2, 3))
        if dpre is not None:
            rdw, rdb = rdw + dpre[0], rdb + dpre[1]
        _check(dw[idx], rdw, F32, gexact, f"{entry} dW")
        _check(db[idx], rdb, F32, gexact, f"{entry} db")
    return pl


# --------------------------------------------------------------------------- the matrices
@pytest.mark.gpu
@pytest.mark.parametrize("row,entry,dt,data", STREAM_CASES)
def test_stream_plan_point(row, entry, dt, data):
    W, H, B, C, band, _ = row
    Cn = 2 * C if entry in GATE else C
    pl = plan(B, Cn, H, W, 3, entry)
    assert pl["family"] == "stream" and pl["band"] == band and pl["lpr"] == W // 4, pl
    assert pl["uni"] == _stream_uni(W, H, band), pl
    run(entry, DTS[dt], B, Cn, H, W, 3, rand=data == "rand", seed=W + H + band)


@pytest.mark.gpu
@pytest.mark.parametrize("row,entry,dt,data", LDS_CASES)
def test_lds_plan_point(row, entry, dt, data):
    W, H, ks, group = row
    C = 4 if group == "gate" else 3
    pl = plan(2, C, H, W, ks, entry)
    tw = 64 if W >= 48 else (32 if W >= 24 else 16)
    assert pl["family"] == "lds" and pl["tw"] == tw, pl
    run(entry, DTS[dt], 2, C, H, W, ks, rand=data == "rand", seed=W + 3 * H + ks)


# --------------------------------------------------------------------------- other routes to the same result
ALT_SHAPES = [(2, 3, 17, 16), (1, 3, 33, 64), (2, 3, 9, 256)]        # (B, C, H, W): streaming-eligible
ALT_ENTRIES = [e for e in ENTRIES if not e.startswith("rc")]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("entry", ALT_ENTRIES)
@pytest.mark.parametrize("shape", ALT_SHAPES, ids=lambda s: "B{}-C{}-H{}-W{}".format(*s))
def test_streaming_shapes_under_mi_dw_lds_and_misaligned(monkeypatch, shape, entry, dt):
    """Streaming-eligible shapes taken by the LDS-tiled kernels two ways - MI_DW_LDS=1, and every activation one element
    off a 16-byte boundary (vec_ok false) - give the fp64 result, as the default path does (exact data: bitwise)."""
    B, C, H, W = shape
    Cn = 2 * C if entry in GATE else C
    assert plan(B, Cn, H, W, 3, entry)["family"] == "stream"
    run(entry, DTS[dt], B, Cn, H, W, 3, seed=5)
    run(entry, DTS[dt], B, Cn, H, W, 3, mem=Offset(), seed=5)
    monkeypatch.setenv("MI_DW_LDS", "1")
    assert plan(B, Cn, H, W, 3, entry)["family"] == "lds"
    run(entry, DTS[dt], B, Cn, H, W, 3, seed=5)


@pytest.mark.gpu
def test_recompute_refuses_what_it_cannot_run(monkeypatch):
    """The recomputing gate backward exists for the streaming plans only: other shapes, kernel sizes and misaligned planes
    are refused with an error (never silently computed some other way)."""
    L, o = lib(), ops()
    x = torch.zeros(2 * 4 * 17 * 64 + 4, device=DEV)
    dx = torch.zeros_like(x)
    w = torch.zeros(4 * 49, device=DEV)
    dw = torch.zeros(4 * 49, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)

    def call(off, H, W, ks):
        return L.mi_dwconv_gate_bwd_recompute(_p(x) + off, _p(x) + off, _p(w), None, _p(dx) + off, _p(dw), None, 2, 4, H, W,
                                              ks, 0, 0, _p(ws), o._stream())
    for H, W, ks in ((17, 13, 3), (5, 24, 3), (17, 64, 5), (17, 64, 7)):
        assert call(0, H, W, ks) != 0
        assert b"mi_dwconv_gate_recompute_ok" in L.mi_last_error()
    assert call(4, 17, 16, 3) != 0                        # 4 bytes off: not 16-byte aligned
    assert call(0, 17, 16, 3) == 0
    monkeypatch.setenv("MI_DW_LDS", "1")
    assert call(0, 17, 16, 3) != 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- bounds and workspace
# (B, C, H, W, ks): one representative shape per plan - band 8 on every row width (the few-plane plans write the most
# partial rows), the UNI form, a taller band, every LDS tile width at 1 and 4 (plain) / 2 (gate) rows per thread, 5x5, 7x7.
BOUNDS = [(2, 3, 17, 16, 3), (2, 3, 23, 32, 3), (3, 3, 9, 64, 3), (2, 3, 16, 128, 3), (2, 3, 5, 256, 3), (2, 3, 128, 16, 3),
          (1, 8193, 17, 128, 3),
          (2, 3, 65, 13, 3), (2, 3, 257, 17, 3), (2, 3, 33, 31, 3), (2, 3, 129, 24, 3), (2, 3, 17, 70, 3),
          (2, 3, 65, 130, 3), (2, 3, 63, 47, 5), (2, 3, 17, 96, 7)]


def _streams(W, ks):
    """The recomputing gate backward exists for these shapes only (mi_dwconv_gate_recompute_ok)."""
    return ks == 3 and W in (16, 32, 64, 128, 256)


BOUNDS_CASES = [pytest.param(c, e, d, id="B{}-C{}-H{}-W{}-k{}".format(*c) + f"-{e}-{d}")
                for c in BOUNDS for e in ENTRIES for d in ("f32", "bf16") if _streams(c[3], c[4]) or not e.startswith("rc")]


def _guard_for(B, C, H, W, ks):
    """A guard wider than anything a wrong plan could reach: a full band past the plane and every plane a lane group of the
    last workgroup could name."""
    return (C + 4 * 16 + 4) * H * W * 4 + 64 * W * 4 + (2 * math.ceil(H / 8) + 2) * C * 10 * 4


@pytest.mark.gpu
@pytest.mark.parametrize("case,entry,dt", BOUNDS_CASES)
def test_bounds_and_workspace(case, entry, dt):
    """Outputs between NaN guards that must stay bitwise unchanged, inputs between NaN margins that must not leak into
    the result, and a workspace of exactly mi_dwconv_bwd_workspace bytes (NaN-filled, guarded behind)."""
    B, C, H, W, ks = case
    Cn = 2 * C if entry in GATE else C
    run(entry, DTS[dt], B, Cn, H, W, ks, mem=Guarded(_guard_for(B, Cn, H, W, ks)), seed=7)


# --------------------------------------------------------------------------- accumulation, deferral, reproducibility
ACC = [(2, 3, 23, 16, 3), (1, 8193, 17, 128, 3), (2, 3, 70, 31, 3), (2, 3, 20, 24, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,entry", [pytest.param(c, e, id="B{}-C{}-H{}-W{}-k{}".format(*c) + f"-{e}")
                                        for c in ACC for e in ("bwd", "gate_bwd", "rc") if e != "rc" or _streams(c[3], c[4])])
def test_accumulate_adds_to_prefilled_gradients(case, entry):
    B, C, H, W, ks = case
    Cn = 2 * C if entry in GATE else C
    pre = (_taps(Cn, ks, 91, False) * 8, _bias(Cn, ks, 92, False) * 8)
    run(entry, F32, B, Cn, H, W, ks, seed=11, acc_prefill=pre)


def _bwd_grads(entry, B, C, H, W, ks, accumulate, rand, seed=13):
    """dW, db of one fp32 backward call (fresh buffers, zero-filled when accumulating).  Integer data keep every sum exact;
    for the gate, y1 in {0, 8} makes gelu(y1) and gelu'(y1) exactly 0 / 0.5 and 8 / 1 in fp32, so d1, d2 are exact too."""
    L, o = lib(), ops()
    x = _data((B, C, H, W), F32, seed, rand)
    d = _data((B, C // 2 if entry != "bwd" else C, H, W), F32, seed + 1, rand)
    y = _data((B, C, H, W), F32, seed + 2, rand)
    if not rand:
        y[:, :C // 2] = 8 * _data((B, C // 2, H, W), F32, seed + 4, False, 0, 1)
    w = _taps(C, ks, seed + 3, rand)
    dx = torch.empty_like(x)
    dw = torch.zeros((C, ks * ks), device=DEV)
    db = torch.zeros((C,), device=DEV)
    ws = torch.empty(L.mi_dwconv_bwd_workspace(B, C, H, W, ks), dtype=torch.uint8, device=DEV)
    if entry == "bwd":
        rc = L.mi_dwconv_bwd(_p(d), _p(x), _p(w), _p(dx), _p(dw), _p(db), B, C, H, W, ks, accumulate, 0, _p(ws), o._stream())
    else:
        rc = L.mi_dwconv_gate_bwd(_p(d), _p(y), _p(x), _p(w), _p(dx), _p(dw), _p(db), B, C, H, W, ks, accumulate, 0, _p(ws),
                                  o._stream())
    _ok(rc, entry)
    return dw, db


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["bwd", "gate_bwd"])
@pytest.mark.parametrize("case", [(8, 4, 256, 16, 3), (8, 4, 300, 70, 3)], ids=["stream-band8-256rows", "lds-tw64"])
def test_deferred_partials_match_the_immediate_reduction(case, entry):
    """With an arena lent (ops.deferred_begin) the partials of an accumulating backward go there and the sum runs at the
    flush: bitwise the immediate result on exact data (the flush sums in an order of its own); and two identical immediate
    calls on random data agree bitwise."""
    B, C, H, W, ks = case
    o = ops()
    fam = "stream" if W == 16 else "lds"
    pl = plan(B, C, H, W, ks, entry)
    assert pl["family"] == fam and (fam == "lds" or pl["band"] == 8 and B * pl["nb"] > 128), pl
    first = _bwd_grads(entry, B, C, H, W, ks, 1, True)
    again = _bwd_grads(entry, B, C, H, W, ks, 1, True)
    torch.cuda.synchronize()
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "two identical calls differ"
    ref = _bwd_grads(entry, B, C, H, W, ks, 1, False)
    tok = o.deferred_begin(4 * lib().mi_dwconv_bwd_workspace(B, C, H, W, ks) + (8 << 20), torch.device(DEV))
    assert tok is not None
    try:
        o.deferred_record(True)
        got = _bwd_grads(entry, B, C, H, W, ks, 1, False)
        assert o.deferred_pending() > 0, "nothing was deferred"
        o.deferred_flush()
    finally:
        o.deferred_end(tok)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


# --------------------------------------------------------------------------- coverage of the tables (no GPU needed)
def test_stream_matrix_is_covered():
    seen = set()
    for W, H, B, C, band, uni in STREAM:
        for op, Cn in (("fwd", C), ("gate_fwd", 2 * C), ("bwd", C), ("gate_bwd", 2 * C)):
            pl = ops().dwconv_plan(B, Cn, H, W, 3, op)
            assert pl["family"] == "stream" and pl["band"] == band, (W, H, op, pl)
            assert uni is None or pl["uni"] == uni, (W, H, op, pl)
            G = 64 // pl["lpr"]
            units = B * (Cn // 2 if op.startswith("gate") else Cn) * pl["nb"]
            seen.add((W, band, pl["uni"], seam(H, band), units % (4 * G) != 0))
        assert max(B * C, B * 2 * C) * H * W * 4 < 1.1e9, "keep every tensor under ~1 GB"
    for W in (16, 32, 64, 128, 256):
        for band in (8, 16, 32, 64):
            assert any(s[0] == W and s[1] == band for s in seen), (W, band)
        assert any(s[0] == W and s[2] for s in seen), f"W={W}: no UNI plan"
        assert W == 256 or any(s[0] == W and not s[2] for s in seen), f"W={W}: no plan without UNI"
        assert any(s[0] == W and s[4] for s in seen), f"W={W}: no partly inactive last workgroup"
    want = {8: {"1", "2", "lt", "kb", "kb+1", "kb+b-1"}, 16: {"kb", "kb+1", "kb+b-1"}, 32: {"kb", "kb+1", "kb+b-1"},
            64: {"1", "2", "lt", "kb", "kb+1", "kb+b-1"}}
    for band, classes in want.items():
        assert classes <= {s[3] for s in seen if s[1] == band}, (band, classes - {s[3] for s in seen if s[1] == band})
    # every entry point at every (W, band) plan point, the seam-bearing entries in both dtypes
    ran = {}
    for i, r in enumerate(STREAM):
        for e, d, dat in _entries_for(i):
            ran.setdefault((r[0], r[4]), set()).add((e, d))
    for key, es in ran.items():
        assert {e for e, _ in es} == set(ENTRIES), key
        for e in CORE:
            assert {(e, "f32"), (e, "bf16")} <= es, key


def test_lds_matrix_is_covered():
    seen = set()
    for W, H, ks, group in LDS:
        for e in (("fwd", "bwd") if group == "plain" else ("gate_fwd", "gate_bwd")):
            pl = ops().dwconv_plan(2, 4, H, W, ks, PLAN_OP[e])
            assert pl["family"] == "lds", (W, H, ks, e, pl)
            th = pl["th"]
            r = H % th
            where = "th" if r == 0 else ("th+1" if r == 1 and H > th else ("th-1" if r == th - 1 else "other"))
            seen.add((pl["tw"], pl["rpt"], ks, where, W % 4 == 0))
    for tw in (16, 32, 64):
        for ks in (3, 5, 7):
            for rpt in ((1, 2, 4) if ks == 3 else (1,)):
                heights = {s[3] for s in seen if s[:3] == (tw, rpt, ks)}
                assert {"th", "th+1"} <= heights, (tw, rpt, ks, heights)
                assert rpt == 2 or "th-1" in heights, (tw, rpt, ks, heights)
    assert {W for W, _, _, _ in LDS} == {5, 13, 17, 24, 31, 47, 48, 70, 96, 130}
    assert any(s[4] for s in seen) and any(not s[4] for s in seen)


def test_plan_query_follows_the_switch_and_rejects_bad_arguments(monkeypatch):
    o = ops()
    for B, C, H, W, ks in BOUNDS + ACC:
        assert o.dwconv_gate_recompute_ok(H, W, ks) == _streams(W, ks)
    assert o.dwconv_plan(2, 6, 17, 16, 3, "gate_bwd") == o.dwconv_plan(2, 3, 17, 16, 3, "bwd")   # gate: B*C/2 planes
    assert o.dwconv_plan(2, 6, 17, 16, 5, "fwd")["family"] == "lds"
    assert o.dwconv_plan(2, 6, 17, 24, 3, "fwd")["family"] == "lds"
    with pytest.raises(RuntimeError):
        o.dwconv_plan(2, 5, 17, 16, 3, "gate_fwd")
    with pytest.raises(RuntimeError):
        o.dwconv_plan(2, 6, 17, 16, 4, "fwd")
    monkeypatch.setenv("MI_DW_LDS", "1")
    assert o.dwconv_plan(2, 6, 17, 16, 3, "fwd") == {"family": "lds", "th": 64, "bands": 1, "tw": 16, "uni": False, "rpt": 1}

"""Case tables, the descriptor builder, the assertions and a CPU model of the 1x1 GEMM (csrc/pw_gemm.hip, csrc/pw_lds.hip).

Shared by tests/test_gpu_pw_forms.py (which runs the kernels) and tests/test_cabi.py (which, without a GPU, checks that the
tables reach every kernel instance and every loop state, that the LayerNorm bar admits correct bf16 arithmetic and that it and
the NaN guard fail on injected faults).  A plain module: no fixtures, no pytest settings.

A ROW is a dict (see row()): the shape, the descriptor features, the MI_PW_* switches, and what ops.pw_plan must say of the call:
the kernel INSTANCE (key(): ("xres", K chunks, fp8), ("stream", tile rows, fp8), ("xwide", K chunks, fp8, LayerNorm),
("resident", tile rows), ("chunked" | "dma", dtype, tile rows), ("lds", tile rows)) and the loop state (pixel tiles per wave /
per workgroup, X-wide slabs, grid, XCD map, weight source, LayerNorm, fp8).  reach() asserts both from the plan of the REAL
descriptor, so a retuned threshold or a switch the planner ignores fails instead of testing the default twice.

Operands are channel slices of wider buffers (batch and group strides exceed the dense extent), and every output lies inside a
buffer pre-filled with NaN: after the call the guard must still be all NaN and the output proper must hold none."""
import ctypes as C
import functools
import math

import torch

from test_gpu_primitives import ints                     # the suite's small-integer data, not a copy of it

# ---------------------------------------------------------------------------------------------- instances and switches
PW_SWITCHES = ("MI_PW_WAVE", "MI_PW_CHUNKED", "MI_PW_DMA", "MI_PW_XWIDE", "MI_PW_WAVE_WIDE", "MI_PW_LDS", "MI_NO_PW_LDS", "MI_PW_DIRECT",
               "MI_PW_B16", "MI_PW_TM_EVEN", "MI_PW_TPB", "MI_PW_WAVE_TPW", "MI_PW_XCD")
PW_WAVE_FORMS = ("xres", "stream", "xwide")
# every instance the launchers can select: (family, tile rows / K chunks, ...).  The weight-resident kernel has a 48-row instance
# that no shape takes: 48-row tiles need M <= 48, and M <= 64 stays chunked.
PW_INSTANCES = (
    {("chunked", dt, tm) for dt in ("f32", "bf16") for tm in (128, 96, 64, 48)} | {("resident", tm) for tm in (128, 96, 64)} |
    {("dma", dt, tm) for dt in ("f32", "bf16") for tm in (128, 64)} | {("xres", kb, f8) for kb in (1, 2, 3) for f8 in (False, True)} |
    {("stream", tm, f8) for tm in (96, 64, 48) for f8 in (False, True)} |
    {("xwide", kb, f8, ln) for kb in (4, 5, 6) for f8 in (False, True) for ln in ((False, True) if kb == 4 else (False,))} |
    {("lds", 256), ("lds", 128)})
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def key(dtype, p):
    """The kernel instance a plan names."""
    dt = "bf16" if dtype == torch.bfloat16 else "f32"
    return {"chunked": (p["family"], dt, p["tm"]), "dma": (p["family"], dt, p["tm"]), "resident": (p["family"], p["tm"]),
            "lds": (p["family"], p["tm"]), "xres": (p["family"], p["kb"], p["f8"]), "stream": (p["family"], p["tm"], p["f8"]),
            "xwide": (p["family"], p["kb"], p["f8"], p["ln"])}[p["family"]]


def set_switches(monkeypatch, env=None):
    for k in PW_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------- rows
T19 = 19 * 64          # 19 pixel tiles: on 8-wave workgroups one wave ends its range inside the plane and whole waves are idle
ROW_DEFAULTS = dict(
    K2=0, B=2, G=1, dtype="bf16", per_image=False, transposed=False, bias=True, res=False, env={}, replaced=None, dense=False,
    x_off=0,                    # elements added to the x1 pointer alone (a pointer-only misalignment)
    split=0,                    # y_split: rows >= split go to y2
    b16=False, wsrc="pack",     # a bf16 copy of per-image weights is given; the weight source the plan must report
    follow="w",                 # with a copy, w holds OTHER values (copy + 1): which of the two the result must follow
    f8=False, ln=0, stats=False,
    tpw=None, tpb=None, grid=None, n_slabs=None, slabs_per=None, xcd=False)   # loop state (None: the family's default, see reach)


def row(inst, M, K, N, **kw):
    unknown = set(kw) - set(ROW_DEFAULTS)
    assert not unknown, unknown
    return {**ROW_DEFAULTS, "key": inst, "M": M, "K": K, "N": N, **kw}


def case_id(r):
    s = ["-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in r["key"]), f"{r['M']}x{r['K']}" + (f"+{r['K2']}" if r["K2"] else ""),
         f"b{r['B']}n{r['N']}"]
    s += [f"g{r['G']}"] if r["G"] > 1 else []
    s += [n for n in ("per_image", "transposed", "bias", "res", "dense", "b16", "stats") if r[n]]
    s += [f"{n}{r[n]}" for n in ("x_off", "split", "ln") if r[n]]
    s += [f"follow_{r['follow']}"] if r["b16"] else []
    s += [f"{k[6:]}={v}" for k, v in sorted(r["env"].items())]
    return "-".join(s)


def both_epilogues(rows):
    """Each row with bias alone and with bias + residual: the two store paths differ."""
    return [{**r, "res": res} for r in rows for res in (False, True)]


XRES_SHAPES = [(1, 100, 24), (2, 144, 48), (3, 254, 96), (3, 510, 96)]       # kb, M, K; 510 x 96 is the shape at the LDS limit
STREAM_SHAPES = [(48, 48, 127), (64, 64, 160), (96, 192, 200)]               # tm, M, K; 192 x 200 has two m-tiles
XWIDE_KS = [(4, 97), (5, 130), (6, 192)]


def _wave_loop_rows():
    out = []
    for f8 in (False, True):
        for tpw, gx in ((2, 2), (3, 1)):     # 16 / 24 tiles per workgroup: ranges of 2 (3) tiles, the last one cut by the plane
            env = {"MI_PW_WAVE_TPW": str(tpw)}
            rep = None if f8 else {"MI_PW_WAVE": "0"}
            out += [row(("xres", kb, f8), M, K, T19, f8=f8, tpw=tpw, grid=(gx, 1, 2), env=env, replaced=rep) for kb, M, K in XRES_SHAPES]
            out += [row(("stream", tm, f8), M, K, T19, f8=f8, tpw=tpw, grid=(gx, -(-M // tm), 2), env=env, replaced=rep)
                    for tm, M, K in STREAM_SHAPES]
    return both_epilogues(out)


WAVE_LOOP_CASES = _wave_loop_rows()

# the workgroup permutation of the stream form (A/B switch, MI_PW_XCD = fewest m-tiles that take it): bit-equal to the plain order
XCD_CASES = [row(("stream", 96, False), 192, 200, 16 * 64, grid=(2, 2, 2), xcd=True, env={"MI_PW_XCD": "1"}, res=True),
             row(("stream", 96, False), 384, 384, 8 * 64, grid=(1, 4, 2), xcd=True, env={"MI_PW_XCD": "2"})]

_RES_OFF = {"MI_PW_WAVE": "0"}
RESIDENT_CASES = both_epilogues(
    # the tile loop: 3 pixel tiles per workgroup on 19 -> 7 workgroups, the last with one tile
    [row(("resident", tm), M, K, T19, tpb=3, grid=(7, -(-M // tm), 2), env={**_RES_OFF, "MI_PW_TPB": "3"}, replaced={"MI_PW_CHUNKED": "1"})
     for tm, M, K in ((128, 128, 100), (96, 192, 100), (96, 288, 96), (64, 144, 48))]
    # a partial pixel tile, default switches: planes of whole 16-byte rows that are no multiple of 64 pixels
    + [row(("resident", 64), 144, 48, 72, tpb=1, grid=(2, 3, 2), replaced={"MI_PW_CHUNKED": "1"}),
       row(("resident", 64), 144, 48, T19 + 8, tpb=1, grid=(20, 3, 2)),
       row(("resident", 128), 128, 100, 72, tpb=1, grid=(2, 1, 2), transposed=True),
       row(("resident", 96), 288, 96, T19 + 8, tpb=2, grid=(10, 3, 2), env={"MI_PW_TPB": "2"}),
       # K = 128 is the last K that stays resident; K = 129 goes to the chunked kernel
       row(("resident", 128), 144, 128, 72, tpb=1, grid=(2, 2, 2)), row(("chunked", "bf16", 128), 144, 129, 72, grid=(2, 2, 2))])

_XW = dict(n_slabs=5)
XWIDE_CASES = both_epilogues(
    # slabs_per == 1 on 19 tiles: 3 workgroups of 8 waves, waves past the plane; every K-chunk count
    [row(("xwide", kb, False, False), 300, K, T19, grid=(3, 5, 2), slabs_per=1, replaced={"MI_PW_XWIDE": "0"}, **_XW) for kb, K in XWIDE_KS]
    + [row(("xwide", 5, False, False), 300, 130, T19, grid=(3, 5, 2), slabs_per=1, per_image=True, transposed=True, **_XW),
       row(("xwide", 5, False, False), 300, 100, T19, K2=30, grid=(3, 5, 2), slabs_per=1, **_XW)])   # the panel seam inside a 32-k chunk
XWIDE_CASES += [
    # the slab pipeline: 5 slabs over 3 workgroups (2, 2, 1: a ragged last one) and all 5 in one (odd count, both buffer parities)
    row(("xwide", 5, False, False), 300, 130, 4096, B=13, grid=(8, 3, 13), slabs_per=2, per_image=True, **_XW),
    row(("xwide", 5, False, False), 300, 100, 4096, K2=30, B=25, grid=(8, 1, 25), slabs_per=5, res=True, **_XW)]

_CH_SHAPES = [(48, 48, 48), (64, 144, 48), (96, 96, 48), (128, 128, 100)]     # tm, M, K
CHUNKED_CASES = (
    [row(("chunked", dt, tm), M, K, 35, dtype=dt, res=True, G=G) for dt in DTYPES for tm, M, K in _CH_SHAPES for G in ((2,) if tm == 48 else (1,))]
    + [row(("chunked", "f32", tm), M, K, 72, dtype="f32", res=True) for tm, M, K in _CH_SHAPES]
    + [row(("chunked", "bf16", tm), M, K, 72, res=True, env={"MI_PW_CHUNKED": "1"}) for tm, M, K in _CH_SHAPES]
    # a pointer-only misalignment: aligned rows and strides, the x view starting one element in -> scalar loads
    + [row(("chunked", dt, 64), 144, 48, 256, dtype=dt, x_off=1, res=True) for dt in DTYPES])
DMA_CASES = [row(("dma", dt, tm), M, K, N, dtype=dt, res=res, env={"MI_PW_DMA": "1"}, replaced={"MI_PW_CHUNKED": "1"})
             for dt in DTYPES for tm, M, K in ((64, 144, 48), (128, 128, 100)) for N, res in ((T19, True), (72, False))]

_ALL = {"MI_PW_LDS": "all"}
LDS_CASES = both_epilogues(
    [row(("lds", 256), 1021, 384, 256, grid=(4, 1, 2), replaced={"MI_NO_PW_LDS": "1"}),
     row(("lds", 256), 192, 576, 256, grid=(1, 1, 2), replaced={"MI_NO_PW_LDS": "1"}, transposed=True),
     row(("lds", 128), 128, 129, 256, grid=(1, 1, 2), env=_ALL, replaced={"MI_NO_PW_LDS": "1"}),
     row(("lds", 128), 300, 129, 264, grid=(3, 2, 2), env=_ALL, replaced={"MI_NO_PW_LDS": "1"})])   # a partial 256-pixel tile

# the split output, one shape per wave family: the split on a row, inside a 16-row fragment, on a 64-row tile seam, on the last row
_SPLIT_SHAPES = [(("xres", 2, False), 144, 48, {}), (("stream", 96, False), 96, 96, {}), (("xwide", 4, False, False), 256, 128, dict(n_slabs=4, slabs_per=1))]
SPLIT_CASES = [row(inst, M, K, T19, split=s, **kw) for inst, M, K, kw in _SPLIT_SHAPES for s in (1, 49, 64, M - 1)]
SPLIT_CASES += [row(inst, M, K, T19, split=49, tpw=2, env={"MI_PW_WAVE_TPW": "2"}) for inst, M, K, kw in _SPLIT_SHAPES[:2]]   # (xwide has no tile loop)

# per-image weight sources.  K = 40: a multiple of 8, not of 32; M with a tile tail; two groups on the narrow shapes; the copy
# has padded rows (w_b16_sm = K + 8) and w holds other values, so the result shows which of the two was read
_WS_SHAPES = [(("xres", 2, False), 100, 40, 2, {}), (("stream", 96, False), 70, 40, 2, {}), (("xwide", 4, False, False), 300, 104, 1, dict(n_slabs=5, slabs_per=1))]
WSRC_CASES = []
for _inst, _M, _K, _G, _kw in _WS_SHAPES:
    _b = dict(per_image=True, G=_G, **_kw)
    WSRC_CASES += [row(_inst, _M, _K, T19, **_b), row(_inst, _M, _K, T19, transposed=True, **_b),
                   row(_inst, _M, _K, T19, wsrc="f32", env={"MI_PW_DIRECT": "1"}, **_b),
                   row(_inst, _M, _K, T19, wsrc="f32", env={"MI_PW_DIRECT": "1"}, transposed=True, res=True, **_b),
                   row(_inst, _M, _K, T19, b16=True, wsrc="b16", follow="b16", **_b),
                   row(_inst, _M, _K, T19, b16=True, wsrc="b16", follow="b16", res=True, **_b),
                   row(_inst, _M, _K, T19, b16=True, wsrc="pack", follow="w", env={"MI_PW_B16": "0"}, **_b)]
WSRC_CASES += [   # K no multiple of 8: the copy cannot be staged in 16-byte pieces, the plan falls back to its own pack
    row(("xres", 2, False), 100, 44, T19, per_image=True, G=2, b16=True, wsrc="pack", follow="w"),
    row(("xwide", 4, False, False), 300, 100, T19, per_image=True, b16=True, wsrc="pack", follow="w", n_slabs=5, slabs_per=1),
    row(("xres", 2, False), 100, 40, T19, per_image=True, G=2, b16=True, wsrc="b16", follow="b16", tpw=2, env={"MI_PW_WAVE_TPW": "2"})]

# fp8 operands at the default switches: e4m3 holds the suite's small integers exactly, so these are exact too
F8_CASES = both_epilogues(
    [row(("xres", kb, True), M, K, T19, f8=True) for kb, M, K in XRES_SHAPES[:3]]
    + [row(("stream", 48, True), 48, 127, T19, f8=True), row(("stream", 64, True), 64, 160, T19, f8=True),
       row(("stream", 96, True), 96, 96, T19, f8=True, G=2), row(("stream", 96, True), 192, 200, T19, f8=True, grid=(3, 2, 2))]
    + [row(("xwide", kb, True, False), 300, K, T19, f8=True, grid=(3, 5, 2), slabs_per=1, **_XW) for kb, K in XWIDE_KS])

# LayerNorm on load: its four instances, both modes, statistics requested and not, K tails (masked statistics); on xres also
# inside the tile loop, where the next tile is prefetched into the registers just normalised in place
LN_CASES = [row(("xres", kb, False), 144, K, T19, ln=mode, stats=st, tpw=tpw, env={"MI_PW_WAVE_TPW": str(tpw)} if tpw > 1 else {})
            for kb, K in ((1, 24), (2, 40), (3, 96)) for mode in (1, 2) for st in (False, True) for tpw in (1, 3)]
LN_CASES += [row(("xwide", 4, False, True), 300, K, T19, ln=mode, stats=st, grid=(3, 5, 2), slabs_per=1, **_XW)
             for K in (97, 128) for mode in (1, 2) for st in (False, True)]
# fp8 operands behind the LayerNorm (the tenth fp8 instance): the normalised operand is no integer, so this row is held to the
# LayerNorm bar, with the e4m3 rounding of both operands in the model
LN_CASES += [row(("xwide", 4, True, True), 300, 97, T19, ln=1, stats=True, f8=True, grid=(3, 5, 2), slabs_per=1, **_XW)]

TABLES = {"wave_loops": WAVE_LOOP_CASES, "xcd": XCD_CASES, "resident": RESIDENT_CASES, "xwide": XWIDE_CASES, "chunked": CHUNKED_CASES,
          "dma": DMA_CASES, "lds": LDS_CASES, "split": SPLIT_CASES, "weights": WSRC_CASES, "f8": F8_CASES, "ln": LN_CASES}


# ---------------------------------------------------------------------------------------------- the descriptor
PAD = {"x1": 8, "x2": 16, "r": 16, "y": 8, "y2": 16}      # channel rows of the wider buffer around each (image, group) slice


def layout(r):
    """name -> (rows, batch stride, group stride, offset of the first element) of every activation operand, in elements."""
    N, G, M = r["N"], r["G"], r["M"]
    rows = {"x1": r["K"], "x2": r["K2"], "r": M if r["res"] else 0, "y": r["split"] or M, "y2": M - r["split"] if r["split"] else 0}
    out = {}
    for name, c in rows.items():
        if c:
            pad = 0 if r["dense"] else PAD[name]
            gs = (c + pad) * N
            out[name] = (c, G * gs, gs, (pad // 2) * N + (r["x_off"] if name == "x1" else 0))
    return out


def describe(ops, r, ptr):
    """The full mi_pw_desc of a row; ptr(name) -> the address of an operand's first element."""
    from image_restoration_amd import _lib as L
    lay, d = layout(r), L.PwDesc()
    M, K, G, B = r["M"], r["K"] + r["K2"], r["G"], r["B"]
    d.x1, d.x1_bs, d.x1_gs, d.k1 = ptr("x1"), lay["x1"][1], lay["x1"][2], r["K"]
    if r["K2"]:
        d.x2, d.x2_bs, d.x2_gs, d.k2 = ptr("x2"), lay["x2"][1], lay["x2"][2], r["K2"]
    ld = K + 8 if r["b16"] else K                          # w's rows are padded like the copy's: both share w_bs / w_gs
    d.w, d.w_gs, d.w_bs = ptr("w"), M * ld, (G * M * ld if r["per_image"] else 0)
    d.w_sm, d.w_sk = (1, M) if r["transposed"] else (ld, 1)
    if r["b16"]:
        d.w_b16, d.w_b16_sm = ptr("w_b16"), ld
    if r["bias"]:
        d.bias, d.bias_gs = ptr("bias"), M + 3
    if r["res"]:
        d.r, d.r_bs, d.r_gs = ptr("r"), lay["r"][1], lay["r"][2]
    d.y, d.y_bs, d.y_gs = ptr("y"), lay["y"][1], lay["y"][2]
    if r["split"]:
        d.y_split, d.y2, d.y2_bs, d.y2_gs = r["split"], ptr("y2"), lay["y2"][1], lay["y2"][2]
    d.m, d.n, d.batch, d.groups, d.dtype = M, r["N"], B, G, ops._dtype_code(DTYPES[r["dtype"]])
    if r["ln"]:
        d.ln_mode, d.ln_w, d.ln_b = r["ln"], ptr("ln_w"), ptr("ln_b")      # beta is given in both modes: BiasFree must ignore it
        if r["stats"]:
            d.ln_mean, d.ln_rstd = ptr("ln_mean"), ptr("ln_rstd")
    if r["f8"]:
        d.f8, d.f8_sx, d.f8_sw = 1, 1.0, 1.0
    return d


def probe(ops, r):
    """The row's descriptor over placeholder pointers (the planner reads pointers for their 16-byte alignment only)."""
    es = 2 if r["dtype"] == "bf16" else 4
    return describe(ops, r, lambda name: ops.PW_PROBE + (r["x_off"] * es if name == "x1" else 0))


def reach(ops, r, d):
    """Assert from the plan of the real descriptor, under the switches now set, that the call runs the row's instance in the
    row's loop state; returns the plan."""
    p = ops.pw_plan(d)
    what = case_id(r)
    assert key(DTYPES[r["dtype"]], p) == r["key"], f"{what}: the plan reaches {key(DTYPES[r['dtype']], p)}, the row is written for {r['key']}"
    fam = p["family"]
    want = {"tpw": r["tpw"] or 1 if fam in PW_WAVE_FORMS else 0, "tpb": r["tpb"] or 1 if fam == "resident" else 0, "xcd_map": r["xcd"],
            "weights": r["wsrc"], "ln": bool(r["ln"]), "f8": r["f8"], "grid": r["grid"] or p["grid"]}
    if fam == "xwide":
        assert r["n_slabs"] and r["slabs_per"], f"{what}: an X-wide row names its slabs"
    want["n_slabs"], want["slabs_per"] = (r["n_slabs"], r["slabs_per"]) if fam == "xwide" else (0, 0)
    got = {k: p[k] for k in want}
    assert got == want, f"{what}: the plan's loop state is {got}, the row is written for {want}"
    return p


def loop_state(r, p):
    """What a row exercises beyond its instance, named for the coverage test of tests/test_cabi.py."""
    s, fam, tiles = set(), p["family"], -(-r["N"] // 64)
    strided = not r["dense"]
    if strided:
        s.add(("strided", fam))
    if fam in ("xres", "stream") and p["tpw"] > 1:
        last = tiles - (p["grid"][0] - 1) * 8 * p["tpw"]          # pixel tiles of the last workgroup, 8 waves
        if last % p["tpw"]:
            s.add(("tpw_ragged", fam))                     # a wave's range ends inside the plane
        if -(-last // p["tpw"]) < 8:
            s.add(("tpw_idle", fam))                       # whole waves have no tile
    if fam == "resident":
        if p["tpb"] > 1 and tiles % p["tpb"]:
            s.add(("tpb_ragged",))
        if r["N"] % 64:
            s.add(("resident_partial_tile",))
    if fam == "xwide":
        sp, ns = p["slabs_per"], p["n_slabs"]
        s.add(("slabs", "one" if sp == 1 else "all" if sp == ns else "some_ragged" if ns % sp else "some"))
    if p["xcd_map"]:
        s.add(("xcd_map",))
    if fam in PW_WAVE_FORMS:
        if r["per_image"]:
            s.add(("weights", p["weights"], fam))
        if r["split"]:
            s.add(("split", fam))
        if p["ln"]:
            s.add(("ln", r["key"][:2], r["ln"]))
    return s


# ---------------------------------------------------------------------------------------------- data and the call
class Call:
    """One mi_pw_gemm call of a row: the descriptor, the tensors behind it, the expected result."""

    def carve(self, name, fill):
        c, bs, gs, off = self.lay[name]
        buf = torch.full((self.r["B"] * bs,), fill, dtype=self.dtype, device=self.device)
        self.bufs[name] = buf
        self.views[name] = buf.as_strided((self.r["B"], self.r["G"], c, self.r["N"]), (bs, gs, self.r["N"], 1), off)
        return self.views[name]

    def ptr(self, name):
        return (self.views[name] if name in self.views else self.tensors[name]).data_ptr()

    def reset_outputs(self):
        for name in self.outputs:
            self.bufs[name].fill_(float("nan"))

    def result(self):
        """The output as fp32 on the CPU, [B, G, M, N] (the two halves of a split output joined)."""
        parts = [self.views[n].float().cpu() for n in ("y", "y2") if n in self.views]
        return torch.cat(parts, 2)

    def check_guards(self):
        for name in self.outputs:
            check_guard(self.bufs[name], self.views[name], f"{case_id(self.r)}: {name}")


def check_guard(buf, view, what=""):
    """The output proper holds no NaN (every element was written) and the buffer around it nothing but NaN (nothing else was)."""
    holes = int(view.isnan().sum())
    assert holes == 0, f"{what}: {holes} elements of the output were never written"
    rest = buf.clone()
    rest.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(float("nan"))
    stray = int((~rest.isnan()).sum())
    assert stray == 0, f"{what}: {stray} elements outside the output were written"


def ln_inputs(B, K, N, seed):
    """Per pixel bf16(mu_p + s_p randn) with mu_p in U(-2, 2), s_p in U(0.5, 2): a statistic applied to the wrong pixel or tile
    shows.  gamma = 1 + 0.3 randn, beta = 0.8 randn, weights bf16(randn / sqrt K) - all as fp32."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.rand((B, 1, 1, N), generator=g) * 4 - 2
    s = torch.rand((B, 1, 1, N), generator=g) * 1.5 + 0.5
    x = (mu + s * torch.randn((B, 1, K, N), generator=g)).to(torch.bfloat16).float()
    gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=g), 0.8 * torch.randn(K, generator=g)
    return x, gamma, beta


@functools.lru_cache(maxsize=4)
def _host(sig):
    """The host tensors of a data signature and the exact fp32 products W x (+ bias), shared by the rows that differ in switches
    or epilogue only.  Small integers: every product and partial sum is exact in fp32 (K <= 2042, |x w| <= 6)."""
    B, G, M, K1, K2, N, per_image, ln = sig
    K = K1 + K2
    h = {}
    if ln:
        h["x1"], h["ln_w"], h["ln_b"] = ln_inputs(B, K1, N, 700 + K1)
        g = torch.Generator().manual_seed(800 + K1)
        h["w"] = (torch.randn((1, G, M, K), generator=g) / math.sqrt(K)).to(torch.bfloat16).float()
        h["bias"] = 0.5 * torch.randn((G, M), generator=g)
    else:
        h["x1"] = ints((B, G, K1, N), 391)
        h["x2"] = ints((B, G, K2, N), 392) if K2 else None
        h["w"] = ints((B if per_image else 1, G, M, K), 393, -2, 3)
        h["bias"] = ints((G, M), 394)
        xs = h["x1"] if not K2 else torch.cat([h["x1"], h["x2"]], 2)
        h["wx"] = torch.einsum("bgmk,bgkn->bgmn", h["w"].expand(B, -1, -1, -1), xs)
        h["wx1"] = h["wx"] + xs.sum(2, keepdim=True)       # (w + 1) x: what a call computes that reads w where w = copy + 1
    h["res"] = ints((B, G, M, N), 395)
    return h


def build(ops, r, device):
    """Allocate a row's operands on `device`, fill them and describe the call."""
    c = Call()
    c.r, c.device, c.dtype, c.lay = r, device, DTYPES[r["dtype"]], dict(layout(r))
    c.bufs, c.views, c.tensors = {}, {}, {}
    B, G, M, K, N = r["B"], r["G"], r["M"], r["K"] + r["K2"], r["N"]
    h = _host((B, G, M, r["K"], r["K2"], N, r["per_image"], bool(r["ln"])))
    c.host = h
    c.carve("x1", 7.0).copy_(h["x1"])                      # (the rows around an input hold a finite value: reads past K meet zero weights)
    if r["K2"]:
        c.carve("x2", 7.0).copy_(h["x2"])
    if r["res"]:
        c.carve("r", 7.0).copy_(h["res"])
    c.outputs = ["y"] + (["y2"] if r["split"] else [])
    for name in c.outputs:
        c.carve(name, float("nan"))
    if r["ln"] and r["stats"]:                             # dense [B, N], in a buffer of one image more: the guard of the statistics
        for name in ("ln_mean", "ln_rstd"):
            c.bufs[name] = torch.full(((B + 1) * N,), float("nan"), device=device)
            c.views[name] = c.bufs[name].as_strided((B, 1, 1, N), (N, N, N, 1), 0)
            c.outputs.append(name)
    w = h["w"]
    if r["b16"]:                                           # rows padded to K + 8; the fp32 matrix holds copy + 1
        pad = torch.full(w.shape[:-1] + (8,), 5.0)
        c.tensors["w_b16"] = torch.cat([w, pad], -1).to(torch.bfloat16).to(device)
        c.tensors["w"] = torch.cat([w + 1.0, pad], -1).to(device)
    else:
        c.tensors["w"] = (w.transpose(-1, -2).contiguous() if r["transposed"] else w).to(device)
    if r["bias"]:
        c.tensors["bias"] = torch.cat([h["bias"], torch.full((G, 3), 9.0)], 1).to(device)
    if r["ln"]:
        c.tensors["ln_w"], c.tensors["ln_b"] = h["ln_w"].to(device), h["ln_b"].to(device)
    c.d = describe(ops, r, c.ptr)
    if not r["ln"]:
        ref = h["wx1"] if (r["b16"] and r["follow"] == "w") else h["wx"]
        if r["bias"]:
            ref = ref + h["bias"][None, :, :, None]
        if r["res"]:
            ref = ref + h["res"]
        c.ref = ref.to(c.dtype).float()                    # rounded once to the output dtype
    return c


# ---------------------------------------------------------------------------------------------- LayerNorm on load: model and bar
CHAIN_FACTOR = 1.5            # the project's own (tests/fused_forms.py)
LN_SLACK = 2.0 ** -8          # one bf16 ulp at the largest magnitude: another fp32 summation order may flip an element's final rounding
BAR_STATS = 1e-5              # statistics against fp64, of the largest magnitude (tests/fused_forms.py)
LN_FAULTS = ("k_tail", "shift", "mode", "tile")


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _e4m3(t):
    return t.to(torch.float8_e4m3fn).to(t.dtype)


def ln_model(h, mode, how, f8=False, fault=None, flip=False):
    """W LN(x) + bias of a LayerNorm row's host tensors, [B, 1, M, N], with the statistics.
    how "fp64": the plain statement R, in fp64 from the bf16 input, the fp32 gamma / beta and the bf16-rounded weights.
    how "kernel": the model E with the kernel's roundings - fp32 two-pass statistics as in ln.hip, the normalised operand rounded
    to bf16 (then to e4m3 with fp8 operands, like the weights), fp32 accumulation, one bf16 rounding of the output.  flip: the
    same in the opposite summation order.
    fault: "k_tail" - the statistics divide by 32 kb, not K; "shift" - gamma / beta shifted by one channel; "mode" - beta applied in
    BiasFree mode and dropped in WithBias mode; "tile" - the statistics of pixel tile t applied to tile t + 1."""
    q = how == "kernel"
    dt = torch.float32 if q else torch.float64
    x, gamma, beta, w, bias = (h[n].to(dt) for n in ("x1", "ln_w", "ln_b", "w", "bias"))
    if flip:
        x, gamma, beta, w = x.flip(2), gamma.flip(0), beta.flip(0), w.flip(3)
    K = x.shape[2]
    inv = torch.tensor(1.0 / (32 * -(-K // 32) if fault == "k_tail" else K), dtype=dt)
    mu = x.sum(2, keepdim=True) * inv
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).sum(2, keepdim=True) * inv + 1e-5)
    mu_u, rstd_u = mu, rstd
    if fault == "tile":
        mu_u, rstd_u = mu.roll(64, 3), rstd.roll(64, 3)
    if fault == "shift":
        gamma, beta = gamma.roll(1), beta.roll(1)
    gv, bv = gamma.view(1, 1, -1, 1), beta.view(1, 1, -1, 1)
    with_beta = (mode == 1) != (fault == "mode")
    xn = (x - mu_u) * rstd_u * gv if mode == 1 else x * rstd_u * gv
    if with_beta:
        xn = xn + bv
    if q:
        xn = _bf(xn)
        if f8:
            xn, w = _e4m3(xn), _e4m3(w)
    y = torch.einsum("bgmk,bgkn->bgmn", w.expand(x.shape[0], -1, -1, -1), xn) + bias[None, :, :, None]
    return (_bf(y) if q else y), mu, rstd


def rel_err(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max())


def ln_bar(e_model):
    return CHAIN_FACTOR * e_model + LN_SLACK


# ---------------------------------------------------------------------------------------------- a CPU stand-in for the wave kernels' stores
def fake_store(call, fault=None):
    """Write a row's expected result into its output buffers the way the wave-owned kernels cover the plane, on the CPU.
    fault "row_past_m": one row more than M is stored; "skipped_tile": the last tile of the first wave's range is never written."""
    r, tpw = call.r, call.r["tpw"] or 1
    y = call.views["y"]
    y.copy_(call.ref)
    if fault == "row_past_m":
        c, bs, gs, off = call.lay["y"]
        call.bufs["y"].as_strided((r["B"], r["G"], 1, r["N"]), (bs, gs, r["N"], 1), off + c * r["N"]).fill_(1.0)
    if fault == "skipped_tile":
        y[..., (tpw - 1) * 64: tpw * 64] = float("nan")

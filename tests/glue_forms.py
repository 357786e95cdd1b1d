"""Case tables, builders, references and assertions of the 3x3 U-Net glue: the implicit-GEMM convolution (csrc/conv3x3.hip:
forward, data gradient, weight gradient) and the layout kernels (csrc/glue.hip: im2col3x3, col2im3x3, pixel_shuffle2, copy_rows).

Shared by tests/test_gpu_glue_forms.py (which runs the kernels) and tests/test_cabi.py (which, without a GPU, checks that the
tables reach every kernel instance and loop state, that every expected value meets the exactness precondition, and that the
assertions fail on results altered the way a broken kernel would alter them).  A plain module: no fixtures, no pytest settings.

A ROW is a dict: the shape, the features of the call, and what the plan query must say of it (the instance and the loop state:
tiles, chunks, splits, bands, blocks, vector).  reach() asserts that from the plan of the real call, so a retuned threshold is a
row that lost its instance, not a kernel that silently went unrun.

Everything is exact.  Operands are small integers (x, dy in [-2, 2], weights in {-1, 0, 1}, bias and residual in [-8, 8], z in
[-3, 3]); the layout kernels move them or add eleven of them, the convolutions contract exact bf16 products in fp32.  Every
expected value is an integer with |y| <= 256 where the output is bf16 and < 2^24 where it is fp32 (precondition(), asserted by
the builders on the reference alone), so the comparison is torch.equal.  Every operand is a slice of a wider buffer filled with
NaN and every output lies inside one: an out-of-bounds read poisons the result, an out-of-bounds write breaks the guard."""
import functools

import torch
import torch.nn.functional as F

from pw_forms import check_guard                         # the suite's guard check, not a copy of it
from test_gpu_primitives import ints                     # the suite's small-integer data, not a copy of it

NAN = float("nan")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
ESIZE = {"f32": 4, "bf16": 2}
VEC = {"f32": 4, "bf16": 8}                              # elements of a 16-byte access
EPILOGUES = ((False, False), (True, False), (False, True), (True, True))      # (bias, residual)

# ---------------------------------------------------------------------------------------------- the instance sets
C3_INSTANCES = {(mt, twp) for mt in (1, 2, 4) for twp in (16, 32, 64)}                      # c3_kernel<MT, TWP>
C3W_INSTANCES = {(twp, swap) for twp in (16, 32, 64) for swap in (False, True)}             # c3_wgrad_kernel<TWP> x row role
G3_STREAM = {(lpr, flip, dt) for lpr in (4, 8, 16, 32, 64) for flip in (False, True) for dt in DTYPES}   # each at band == 8
G3_BANDS = {(64, 16), (64, 32)}                                                                           # (lpr, band), bf16
PS_INSTANCES = {(v, un, dt) for v in ("vector", "element") for un in (False, True) for dt in DTYPES}
CR_INSTANCES = {(v, dt) for v in ("vector", "element") for dt in DTYPES}


def precondition(ref, dtype, what):
    """Every expected value is an integer that the output dtype holds exactly."""
    r = ref.double()
    assert bool((r == r.round()).all()), f"{what}: the reference holds non-integers"
    peak = float(r.abs().max()) if r.numel() else 0.0
    assert peak <= 256 if dtype == torch.bfloat16 else peak < 2 ** 24, f"{what}: peak {peak} is not exact in {dtype}"


def case_id(r):
    skip = ("table", "tiles", "tiles_x", "tiles_y", "chunks", "co_tiles", "splits", "blocks", "bands", "grid")
    out = [r["table"]]
    for k, v in r.items():
        if k in skip or v is None or v is False or v == 0 and k in ("x_off", "out_off", "bs_extra"):
            continue
        out.append(k if v is True else f"{k}{v}")
    return "-".join(out)


# ---------------------------------------------------------------------------------------------- conv forward / data gradient
C3_M = {1: (1, 3, 16), 2: (17, 32), 4: (33, 49, 64, 65)}          # the edges of each m-tile bin
C3_W = {16: (("exact", 16), ("partial", 8)), 32: (("exact", 32), ("partial", 24)),
        64: (("exact", 64), ("partial", 40), ("full+partial", 72), ("two", 128))}
C3_K = (1, 3, 15, 16, 17, 33)
C3_H = ("1", "tr-1", "tr", "tr+1", "2tr+1")
C3_TILES_X = {"exact": 1, "partial": 1, "full+partial": 2, "two": 2}
C3_TILES_Y = {"1": 1, "tr-1": 1, "tr": 1, "tr+1": 2, "2tr+1": 3}
C3_CHUNKS = {1: 1, 3: 1, 15: 1, 16: 1, 17: 2, 33: 3}
C3_CO_TILES = {1: 1, 3: 1, 16: 1, 17: 1, 32: 1, 33: 1, 49: 1, 64: 1, 65: 2}       # 65: a one-row last channel tile


def h_of(kind, tr):
    return {"1": 1, "tr-1": tr - 1, "tr": tr, "tr+1": tr + 1, "2tr+1": 2 * tr + 1}[kind]


def _conv_rows():
    rows = []
    for mt in (1, 2, 4):
        for twp in (16, 32, 64):
            Ms, Ws, tr = C3_M[mt], C3_W[twp], 256 // twp
            for i in range(6):
                wkind, W = Ws[i % len(Ws)]
                hkind = C3_H[(i + 1) % 5]
                bias, res = EPILOGUES[i % 4]
                rows.append(dict(table="conv", mt=mt, twp=twp, B=(1, 3)[(i // 2) % 2], M=Ms[(i + i // len(Ms)) % len(Ms)],
                                 K=C3_K[(i + 2) % 6], H=h_of(hkind, tr), W=W, wkind=wkind, hkind=hkind, bias=bias, res=res,
                                 transpose=False))
            # the data gradient: the flipped, transposed pack; M != K so that swapped pack strides cannot cancel
            for M, K, (wkind, W), hkind, B in ((Ms[-1], 17, Ws[-1], "2tr+1", 3), (Ms[0], 3, Ws[0], "tr-1", 1)):
                rows.append(dict(table="conv", mt=mt, twp=twp, B=B, M=M, K=K, H=h_of(hkind, tr), W=W, wkind=wkind, hkind=hkind,
                                 bias=False, res=False, transpose=True))
    return rows


CONV_CASES = _conv_rows()


def module_route(r):
    """_Conv3x3Fn hands the row to the implicit GEMM (cout >= 16; the row is a plain forward)."""
    return r["table"] == "conv" and not r["transpose"] and r["M"] >= 16


# ---------------------------------------------------------------------------------------------- conv weight gradient
# (B, H, W) per tile width: tiles and splits of each loop state.  tiles = B * tiles_x * tiles_y; the split count is tiles / 2
# here (few 64 x 16 blocks), so split s walks tiles s, s + splits, ...
C3W_LOOPS = ("one", "three", "4/2", "5/2", "7/3", "3x2/3", "past_h")
C3W_TILES = {"one": (1, 1), "three": (3, 1), "4/2": (4, 2), "5/2": (5, 2), "7/3": (7, 3), "3x2/3": (6, 3), "past_h": (2, 1)}
C3W_SHAPES = {
    16: {"one": (1, 16, 16), "three": (1, 48, 8), "4/2": (2, 32, 16), "5/2": (1, 80, 16), "7/3": (7, 16, 8), "3x2/3": (3, 32, 16),
         "past_h": (1, 17, 16)},
    32: {"one": (1, 8, 32), "three": (3, 8, 24), "4/2": (2, 16, 32), "5/2": (5, 8, 32), "7/3": (1, 56, 24), "3x2/3": (3, 16, 32),
         "past_h": (1, 9, 32)},
    64: {"one": (1, 4, 64), "three": (1, 12, 40), "4/2": (1, 8, 128), "5/2": (5, 4, 64), "7/3": (7, 4, 40), "3x2/3": (3, 4, 72),
         "past_h": (1, 5, 64)}}
# (rows, columns) as the kernel sees them after the swap.  The x operand takes the 64-row role only when that pads less:
# ceil(rows / 64) ceil(cols / 16) < ceil(rows / 16) for cols <= 64 - never for rows <= 16, so w_swap rows start at 17
C3W_RC = {False: ((1, 1), (16, 15), (17, 17), (33, 16), (64, 17), (65, 15), (1, 16)),
          True: ((17, 1), (33, 15), (64, 16), (65, 17), (17, 16), (33, 17), (64, 15))}


def _wgrad_rows():
    rows = []
    for twp in (16, 32, 64):
        for swap in (False, True):
            for loop, (rws, cls) in zip(C3W_LOOPS, C3W_RC[swap]):
                B, H, W = C3W_SHAPES[twp][loop]
                M, K = (cls, rws) if swap else (rws, cls)
                tiles, splits = C3W_TILES[loop]
                rows.append(dict(table="wgrad", twp=twp, swap=swap, loop=loop, B=B, M=M, K=K, H=H, W=W, rows=rws, cols=cls,
                                 tiles=tiles, splits=splits, grid=(-(-cls // 16), -(-rws // 64)), accumulate=loop in ("4/2", "7/3")))
    # the other bound of the split count: 128 blocks of 64 x 16 -> ceil(1024 / 128) = 8 splits, fewer than tiles / 2 = 9
    rows.append(dict(table="wgrad", twp=16, swap=False, loop="by_blocks", B=18, M=512, K=256, H=1, W=8, rows=512, cols=256, tiles=18,
                     splits=8, grid=(16, 8), accumulate=False))
    return rows


WGRAD_CASES = _wgrad_rows()

# ---------------------------------------------------------------------------------------------- im2col / col2im
G3_H = (1, 7, 8, 9, 17)                                   # band seams and tails at band 8
_G3_DEFAULTS = dict(x_off=0, out_off=0, bias=False, res=False, device_ref=False, idle=False, trips=1)


def _glue_rows(op):
    """op "im2col": planes = B * C inputs; "col2im": planes = B * M outputs, bias[plane % M] with M > 1."""
    B, Cn = (1, 3) if op == "im2col" else (3, 3)
    rows, n = [], 0
    for lpr in (4, 8, 16, 32, 64):
        for flip in (False, True):
            for dt in DTYPES:
                for _ in range(2):                         # two heights per instance: all five at every row width
                    H = G3_H[n % 5]
                    bias, res = EPILOGUES[n % 4] if op == "col2im" else (False, False)
                    # 3 (9) planes: the last wave of the grid holds idle units at every height
                    rows.append(dict(_G3_DEFAULTS, table=op, form="stream", lpr=lpr, band=8, bands=-(-H // 8), flip=flip, dtype=dt,
                                     B=B, C=Cn, H=H, W=4 * lpr, bias=bias, res=res, idle=True))
                    n += 1
    # taller bands at the smallest plane counts that take them; compared on the device
    for H, band in ((17, 16), (33, 32)):
        rows.append(dict(_G3_DEFAULTS, table=op, form="stream", lpr=64, band=band, bands=-(-H // band), flip=op == "col2im", dtype="bf16",
                         B=8, C=256, H=H, W=256, bias=op == "col2im", res=op == "col2im", device_ref=True))
    # the general form: any width and height
    for W in (1, 3, 8, 20, 24):
        for H in (1, 2, 5):
            bias, res = EPILOGUES[n % 4] if op == "col2im" else (False, False)
            rows.append(dict(_G3_DEFAULTS, table=op, form="general", lpr=0, band=0, bands=0, flip=bool(n % 2), dtype=("f32", "bf16")[n // 2 % 2],
                             B=2, C=3, H=H, W=W, bias=bias, res=res))
            n += 1
    # a streaming width on a pointer 2 (bf16) / 4 (fp32) bytes off a 16-byte boundary: input alone, output alone
    for dt in DTYPES:
        for x_off, out_off in ((1, 0), (0, 1)):
            rows.append(dict(_G3_DEFAULTS, table=op, form="general", lpr=0, band=0, bands=0, flip=x_off == 1, dtype=dt, B=1, C=3, H=9, W=64,
                             x_off=x_off, out_off=out_off, bias=op == "col2im", res=False))
    # past the grid cap of 65536 blocks: the grid-stride loop makes a second trip
    if op == "im2col":
        rows.append(dict(_G3_DEFAULTS, table=op, form="general", lpr=0, band=0, bands=0, flip=True, dtype="bf16", B=1, C=8, H=500, W=500,
                         trips=2, device_ref=True))
    else:
        rows.append(dict(_G3_DEFAULTS, table=op, form="general", lpr=0, band=0, bands=0, flip=False, dtype="bf16", B=4, C=17, H=500, W=500,
                         bias=True, res=True, trips=2, device_ref=True))
    return rows


IM2COL_CASES = _glue_rows("im2col")
COL2IM_CASES = _glue_rows("col2im")

# ---------------------------------------------------------------------------------------------- pixel_shuffle2 / copy_rows
_PS_DEFAULTS = dict(B=2, c=3, x_off=0, out_off=0, bs_extra=0, trips=1)


def _shuffle_rows():
    rows = []
    for un in (False, True):
        for dt in DTYPES:
            V = VEC[dt]
            base = dict(_PS_DEFAULTS, table="shuffle", unshuffle=un, dtype=dt)
            rows += [dict(base, form="vector", H=5, W=2 * V),                           # c, H, W: the low-resolution side
                     dict(base, form="vector", H=1, W=V, B=3, c=1),
                     dict(base, form="element", why="width", H=3, W=V + V // 2),         # W no multiple of the vector
                     dict(base, form="element", why="in_ptr", H=3, W=V, x_off=1),        # a misaligned base pointer, input
                     dict(base, form="element", why="out_ptr", H=3, W=V, out_off=1),     # ... and output
                     dict(base, form="element", why="stride", H=3, W=V, bs_extra=1)]     # a batch stride no multiple of the vector
    # element-wise past 16384 x 256 threads: the grid-stride loop makes a second trip
    rows.append(dict(_PS_DEFAULTS, table="shuffle", unshuffle=False, dtype="bf16", form="element", why="width", H=600, W=601, trips=2))
    return rows


def _copy_rows():
    rows = []
    for dt in DTYPES:
        V = VEC[dt]
        base = dict(_PS_DEFAULTS, table="copy", dtype=dt, trips=1)
        rows += [dict(base, form="vector", c=3, H=5, W=2 * V),
                 dict(base, form="vector", c=1, H=1, W=V, B=3),
                 dict(base, form="element", why="tail", c=3, H=3, W=V + 1),              # L with a vector tail
                 dict(base, form="element", why="in_ptr", c=3, H=3, W=V, x_off=1),
                 dict(base, form="element", why="out_ptr", c=3, H=3, W=V, out_off=1),
                 dict(base, form="element", why="stride", c=3, H=3, W=V, bs_extra=1)]
    return rows


SHUFFLE_CASES = _shuffle_rows()
COPY_CASES = _copy_rows()

TABLES = {"conv": CONV_CASES, "wgrad": WGRAD_CASES, "im2col": IM2COL_CASES, "col2im": COL2IM_CASES, "shuffle": SHUFFLE_CASES,
          "copy": COPY_CASES}


# ---------------------------------------------------------------------------------------------- buffers
def carve_stride(shape, bs_extra=0, front=1, back=2):
    return (front + shape[1] + back) * shape[2] * shape[3] + bs_extra


def carve4(shape, dtype, device, fill=NAN, off=0, bs_extra=0, front=1, back=2):
    """A [B, C, H, W] channel slice (dense [C, H, W] blocks) of a wider buffer filled with `fill`: `front` / `back` guard channels
    around it in every image, the first element on a 16-byte boundary plus `off` elements, the batch stride `bs_extra` wider."""
    B, Cn, H, W = shape
    HW = H * W
    bs = carve_stride(shape, bs_extra, front, back)
    lead = (-front * HW) % 8
    buf = torch.full((lead + off + B * bs,), fill, dtype=dtype, device=device)
    return buf, buf.as_strided(shape, (bs, HW, W, 1), lead + off + front * HW)


def carve_flat(shape, dtype, device, fill=NAN, off=0, guard=64):
    """A dense tensor inside a flat buffer filled with `fill`, `guard` elements before and after (+ `off`: a misaligned pointer)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((guard + off + n + guard,), fill, dtype=dtype, device=device)
    return buf, buf[guard + off: guard + off + n].view(shape)


def aligned16(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


class Call:
    """One call of a row: its operands (views into guarded buffers), the output buffer and view, the reference, the plan."""

    def reset(self):
        self.out_buf.fill_(NAN)
        if getattr(self, "base", None) is not None:
            self.out.copy_(self.base)

    def check(self, got=None):
        """Guards, then bit-for-bit equality; on a mismatch the count of differing elements and the first one with its plan
        coordinates."""
        got = self.out if got is None else got
        who = case_id(self.r)
        check_guard(self.out_buf, self.out, who)
        ref = self.ref.to(device=got.device, dtype=got.dtype)
        if torch.equal(got, ref):
            return
        bad = (got != ref).nonzero()
        idx = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{who}: {bad.shape[0]} of {ref.numel()} elements differ; first at {self.names} = {idx}: got "
                             f"{float(got[idx])}, expected {float(ref[idx])} ({self.locate(idx)})")


# ---------------------------------------------------------------------------------------------- conv: references, builders
def conv_ref(x, w, transpose):
    """float64 on the CPU.  transpose: w is the conv's own [K, M, 3, 3] and the result its data gradient for x."""
    return F.conv_transpose2d(x.double(), w.double(), padding=1) if transpose else F.conv2d(x.double(), w.double(), padding=1)


@functools.lru_cache(maxsize=8)
def _conv_host(B, M, K, H, W, transpose):
    h = {"x": ints((B, K, H, W), 611, -2, 3), "w": ints((K, M, 3, 3) if transpose else (M, K, 3, 3), 612, -1, 2),
         "bias": ints((M,), 613, -8, 9), "res": ints((B, M, H, W), 614, -8, 9), "dy": ints((B, M, H, W), 615, -2, 3)}
    h["y0"] = conv_ref(h["x"], h["w"], transpose)
    return h


def conv_expected(h, r, y0=None):
    y = h["y0"] if y0 is None else y0
    if r["bias"]:
        y = y + h["bias"].double().view(1, -1, 1, 1)
    if r["res"]:
        y = y + h["res"].double()
    return y


def _conv_locate(r, p):
    def f(idx):
        b, m, y, x = idx
        return (f"tile x {x // p['twp']} y {y // p['tr']} of {p['tiles_x']} x {p['tiles_y']}, column {x % p['twp']} row {y % p['tr']}; channel tile "
                f"{m // (16 * p['mt'])} of {p['co_tiles']}, m-tile {m // 16 % p['mt']} row {m % 16}; {p['chunks']} chunks")
    return f


def build_conv(ops, r, device):
    c = Call()
    c.r, c.names = r, "(b, channel, y, x)"
    B, M, K, H, W = (r[k] for k in "BMKHW")
    h = c.host = _conv_host(B, M, K, H, W, r["transpose"])
    bf = torch.bfloat16
    c.x = carve4((B, K, H, W), bf, device)[1].copy_(h["x"])
    c.w = carve_flat(h["w"].shape, torch.float32, device)[1].copy_(h["w"])
    c.bias = carve_flat((M,), torch.float32, device)[1].copy_(h["bias"]) if r["bias"] else None
    c.res = carve4((B, M, H, W), bf, device, front=2, back=1)[1].copy_(h["res"]) if r["res"] else None
    c.out_buf, c.out = carve4((B, M, H, W), bf, device, front=3, back=1)
    c.ref = conv_expected(h, r)
    precondition(c.ref, bf, case_id(r))
    c.plan = ops.conv3x3_plan(B, M, K, H, W)
    c.locate = _conv_locate(r, c.plan)
    return c


def run_conv(ops, c):
    c.reset()
    got = ops.conv3x3(c.x, c.w, c.bias, c.res, transpose=c.r["transpose"], out=c.out)
    assert got.data_ptr() == c.out.data_ptr()
    return c


def wgrad_ref(dy, x):
    w = torch.zeros((dy.shape[1], x.shape[1], 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, padding=1).backward(dy.double())
    return w.grad


@functools.lru_cache(maxsize=8)
def _wgrad_host(B, M, K, H, W):
    h = {"x": ints((B, K, H, W), 621, -2, 3), "dy": ints((B, M, H, W), 622, -2, 3), "base": ints((M, K, 3, 3), 623, -8, 9)}
    h["dw"] = wgrad_ref(h["dy"], h["x"])
    return h


def _wgrad_locate(r, p):
    def f(idx):
        m, k, ky, kx = idx
        row, col = (k, m) if p["w_swap"] else (m, k)
        return (f"tap {3 * ky + kx}; kernel row {row} (block {row // 64} of {p['w_grid_y']}, wave pair {row % 64 // 32}), column {col} (chunk "
                f"{col // 16} of {p['w_grid_x']}); {p['w_splits']} splits, swap {p['w_swap']}")
    return f


def build_wgrad(ops, r, device):
    c = Call()
    c.r, c.names = r, "(m, k, ky, kx)"
    B, M, K, H, W = (r[k] for k in "BMKHW")
    h = c.host = _wgrad_host(B, M, K, H, W)
    bf = torch.bfloat16
    c.dy = carve4((B, M, H, W), bf, device)[1].copy_(h["dy"])
    c.x = carve4((B, K, H, W), bf, device, front=2, back=1)[1].copy_(h["x"])
    c.out_buf, c.out = carve_flat((M, K, 3, 3), torch.float32, device)
    c.base = h["base"] if r["accumulate"] else None          # overwrite: dw itself starts as NaN
    c.ref = h["dw"] + (h["base"].double() if r["accumulate"] else 0)
    precondition(c.ref, torch.float32, case_id(r))
    c.plan = ops.conv3x3_plan(B, M, K, H, W)
    c.locate = _wgrad_locate(r, c.plan)
    return c


def run_wgrad(ops, c):
    c.reset()
    ops.conv3x3_wgrad(c.dy, c.x, c.out, accumulate=c.r["accumulate"])
    return c


# ---------------------------------------------------------------------------------------------- im2col / col2im
def im2col_ref(x, flip):
    """[B, C, H, W] -> [B, 9C, H, W], col[c * 9 + ky * 3 + kx][y][x] = x[c][y + ky - 1][x + kx - 1], the shifts negated when flip."""
    H, W = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1))
    taps = [xp[..., ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]
    return torch.stack(taps[::-1] if flip else taps, 2).flatten(1, 2)


def col2im_ref(z, bias, res, flip):
    """[B, 9M, H, W] -> [B, M, H, W], y[m][y][x] = sum over taps of z[m * 9 + tap][y + ky - 1][x + kx - 1] (+ bias[m]) (+ residual);
    flip: the plane of the opposite tap."""
    B, M9, H, W = z.shape
    zz = z.view(B, M9 // 9, 9, H, W)
    zp = F.pad(zz.flip(2) if flip else zz, (1, 1, 1, 1))
    y = sum(zp[:, :, 3 * ky + kx, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3))
    if bias is not None:
        y = y + bias.to(y.dtype).view(1, -1, 1, 1)
    return y if res is None else y + res.to(y.dtype)


def _g3_data(shape, seed, lo, hi, r, device):
    """Small integers as fp32: from the suite's CPU generator, or drawn on the device for the two big band cases and the cap cases."""
    if r["device_ref"]:
        g = torch.Generator(device=device).manual_seed(seed)
        return torch.randint(lo, hi, shape, generator=g, device=device).float()
    return ints(shape, seed, lo, hi)


def _g3_locate(r, p):
    def f(idx):
        b, ch, y, x = idx
        if not p["fast"]:
            return "general form"
        per_image = r["C"] * (9 if r["table"] == "im2col" else 1)
        return f"plane {b * per_image + ch}, band {y // p['band']} of {p['bands']} row {y % p['band']}, lane {x // 4} of {p['lpr']}"
    return f


def glue_planes(r):
    return r["B"] * r["C"]


def build_glue(ops, r, device):
    """im2col: x [B, C, H, W] -> out [B, 9C, H, W]; col2im: z [B, 9C, H, W] (+ bias [C]) (+ residual) -> out [B, C, H, W]."""
    c = Call()
    c.r, c.names = r, "(b, plane, y, x)"
    B, Cn, H, W = r["B"], r["C"], r["H"], r["W"]
    dt = DTYPES[r["dtype"]]
    where = device if r["device_ref"] else "cpu"
    hi = torch.float32 if r["device_ref"] else torch.float64
    c.bias = c.res = None
    if r["table"] == "im2col":
        x = _g3_data((B, Cn, H, W), 631, -2, 3, r, where)
        c.x = carve_flat((B, Cn, H, W), dt, device, off=r["x_off"])[1].copy_(x)
        c.out_buf, c.out = carve_flat((B, 9 * Cn, H, W), dt, device, off=r["out_off"])
        c.ref = im2col_ref(x.to(hi), r["flip"])
    else:
        z = _g3_data((B, 9 * Cn, H, W), 632, -3, 4, r, where)
        c.x = carve_flat((B, 9 * Cn, H, W), dt, device, off=r["x_off"])[1].copy_(z)
        bias = res = None
        if r["bias"]:
            bias = ints((Cn,), 633, -8, 9)
            c.bias = carve_flat((Cn,), torch.float32, device)[1].copy_(bias)
        if r["res"]:
            res = _g3_data((B, Cn, H, W), 634, -8, 9, r, where)
            c.res = carve_flat((B, Cn, H, W), dt, device)[1].copy_(res)
        c.out_buf, c.out = carve_flat((B, Cn, H, W), dt, device, off=r["out_off"])
        c.ref = col2im_ref(z.to(hi), None if bias is None else bias.to(where), None if res is None else res.to(hi), r["flip"])
    precondition(c.ref, dt, case_id(r))
    c.aligned = aligned16(c.x, c.out, c.res)
    c.plan = ops.glue3x3_plan(glue_planes(r), H, W, dt, c.aligned)
    c.locate = _g3_locate(r, c.plan)
    return c


def run_glue(ops, c):
    from image_restoration_amd import _lib as L
    r = c.r
    c.reset()
    code = ops._dtype_code(DTYPES[r["dtype"]])
    if r["table"] == "im2col":
        L.check(L.lib().mi_im2col3x3(c.x.data_ptr(), c.out.data_ptr(), r["B"], r["C"], r["H"], r["W"], int(r["flip"]), code, ops._stream()),
                "im2col3x3")
    else:
        L.check(L.lib().mi_col2im3x3(c.x.data_ptr(), ops._p(c.bias), ops._p(c.res), c.out.data_ptr(), r["B"], r["C"], r["H"], r["W"],
                                     int(r["flip"]), code, ops._stream()), "col2im3x3")
    return c


# ---------------------------------------------------------------------------------------------- pixel_shuffle2 / copy_rows
def shuffle_ref(x, unshuffle):
    return F.pixel_unshuffle(x, 2) if unshuffle else F.pixel_shuffle(x, 2)


MOVE_IN, MOVE_OUT = dict(front=1, back=2), dict(front=2, back=1)      # guard channels around the input / output slice


def move_shapes(r):
    B, cc, H, W = r["B"], r["c"], r["H"], r["W"]
    if r["table"] == "copy":
        return (B, cc, H, W), (B, cc, H, W)
    lo, hi = (B, 4 * cc, H, W), (B, cc, 2 * H, 2 * W)
    return (hi, lo) if r["unshuffle"] else (lo, hi)


def build_move(ops, r, device):
    """pixel_shuffle2 and copy_rows: input and output are channel slices of wider buffers (the _UpCatFn use)."""
    c = Call()
    c.r, c.names = r, "(b, channel, y, x)"
    B, cc, H, W = r["B"], r["c"], r["H"], r["W"]
    dt = DTYPES[r["dtype"]]
    in_shape, out_shape = move_shapes(r)
    x = ints(in_shape, 641, -2, 3)
    c.x = carve4(in_shape, dt, device, off=r["x_off"], bs_extra=r["bs_extra"], **MOVE_IN)[1].copy_(x)
    c.out_buf, c.out = carve4(out_shape, dt, device, off=r["out_off"], bs_extra=r["bs_extra"], **MOVE_OUT)
    c.ref = x if r["table"] == "copy" else shuffle_ref(x, r["unshuffle"])
    precondition(c.ref, dt, case_id(r))
    c.aligned = aligned16(c.x, c.out)
    if r["table"] == "copy":
        c.plan = ops.copy_rows_plan(B, cc * H * W, c.x.stride(0), c.out.stride(0), dt, c.aligned)
    else:
        c.plan = ops.pixel_shuffle2_plan(B, cc, H, W, c.x.stride(0), c.out.stride(0), dt, c.aligned)
    c.locate = lambda idx: f"vector {c.plan['vector']}, {c.plan['blocks']} blocks"
    return c


def run_move(ops, c):
    c.reset()
    if c.r["table"] == "copy":
        ops.copy_rows(c.x, c.out)
    else:
        ops.pixel_shuffle2(c.x, c.r["unshuffle"], out=c.out)
    return c


BUILD = {"conv": build_conv, "wgrad": build_wgrad, "im2col": build_glue, "col2im": build_glue, "shuffle": build_move, "copy": build_move}
RUN = {"conv": run_conv, "wgrad": run_wgrad, "im2col": run_glue, "col2im": run_glue, "shuffle": run_move, "copy": run_move}


# ---------------------------------------------------------------------------------------------- reach
def row_aligned(r):
    """Whether the pointers the row describes lie on 16-byte boundaries (the builders put every operand there but for x_off / out_off;
    a batch stride that is no multiple of the vector is the launcher's own test)."""
    return (r["x_off"] * ESIZE[r["dtype"]]) % 16 == 0 and (r["out_off"] * ESIZE[r["dtype"]]) % 16 == 0


def instance(r, p):
    """The kernel instance a plan names for a row."""
    t = r["table"]
    if t == "conv":
        return (p["mt"], p["twp"])
    if t == "wgrad":
        return (p["twp"], p["w_swap"])
    if t in ("im2col", "col2im"):
        if not p["fast"]:
            return ("general", r["dtype"])
        return (p["lpr"], r["flip"], r["dtype"]) if p["band"] == 8 else (p["lpr"], p["band"])
    form = "vector" if p["vector"] > 1 else "element"
    return (form, r["unshuffle"], r["dtype"]) if t == "shuffle" else (form, r["dtype"])


def reach(ops, r, aligned=None):
    """Assert from the plan of the real call that the row lands in the instance, the loop state and the alignment form it names;
    returns the plan.  aligned: of the call's real pointers (None: as the row describes them)."""
    who, t = case_id(r), r["table"]
    if t in ("conv", "wgrad"):
        p = ops.conv3x3_plan(r["B"], r["M"], r["K"], r["H"], r["W"])
        if t == "conv":
            want = {"mt": r["mt"], "twp": r["twp"], "tr": 256 // r["twp"], "tiles_x": C3_TILES_X[r["wkind"]], "tiles_y": C3_TILES_Y[r["hkind"]],
                    "co_tiles": C3_CO_TILES[r["M"]], "chunks": C3_CHUNKS[r["K"]]}
        else:
            want = {"twp": r["twp"], "w_swap": r["swap"], "w_rows": r["rows"], "w_cols": r["cols"], "w_splits": r["splits"],
                    "w_grid_x": r["grid"][0], "w_grid_y": r["grid"][1], "w_workspace": r["splits"] * r["M"] * r["K"] * 36}
            assert r["B"] * p["tiles_x"] * p["tiles_y"] == r["tiles"], f"{who}: {r['B']} x {p['tiles_x']} x {p['tiles_y']} tiles, the row names {r['tiles']}"
    elif t in ("im2col", "col2im"):
        al = row_aligned(r) if aligned is None else aligned
        assert al == row_aligned(r), f"{who}: the call's pointers are {'aligned' if al else 'misaligned'}, the row describes the opposite"
        dt, planes = DTYPES[r["dtype"]], glue_planes(r)
        p = ops.glue3x3_plan(planes, r["H"], r["W"], dt, al)
        want = {"fast": r["form"] == "stream", "lpr": r["lpr"], "band": r["band"], "bands": r["bands"]}
        mine = "blocks_" + t
        if p["fast"]:
            units, per_block = planes * p["bands"], 4 * (64 // p["lpr"])
            want[mine] = -(-units // per_block)
            assert (units % per_block != 0) == r["idle"], f"{who}: {units} units on blocks of {per_block}, idle lanes named {r['idle']}"
        else:
            outputs = planes * r["H"] * r["W"] * (9 if t == "im2col" else 1)
            want[mine] = min(outputs // 256 + 1, 65536)
            assert (outputs > 65536 * 256) == (r["trips"] == 2), f"{who}: {outputs} outputs, the row names {r['trips']} trips"
    else:
        al = row_aligned(r) if aligned is None else aligned
        assert al == row_aligned(r), f"{who}: the call's pointers are {'aligned' if al else 'misaligned'}, the row describes the opposite"
        dt, B, cc, H, W = DTYPES[r["dtype"]], r["B"], r["c"], r["H"], r["W"]
        HW = H * W
        in_shape, out_shape = move_shapes(r)
        bs_in, bs_out = carve_stride(in_shape, r["bs_extra"], **MOVE_IN), carve_stride(out_shape, r["bs_extra"], **MOVE_OUT)
        if t == "copy":
            p = ops.copy_rows_plan(B, cc * HW, bs_in, bs_out, dt, al)
            items = B * cc * HW
        else:
            p = ops.pixel_shuffle2_plan(B, cc, H, W, bs_in, bs_out, dt, al)
            items = B * cc * 2 * HW
        v = VEC[r["dtype"]] if r["form"] == "vector" else 1
        want = {"vector": v, "total": items // v, "blocks": min(-(-(items // v) // 256), 16384)}
        assert (want["total"] > 16384 * 256) == (r["trips"] == 2), f"{who}: {want['total']} work items, the row names {r['trips']} trips"
    got = {k: p[k] for k in want}
    assert got == want, f"{who}: the plan says {got}, the row is written for {want}"
    return p


# ---------------------------------------------------------------------------------------------- deliberately wrong results
def tile_of(p, B, H, W):
    """[B, H, W] map of the weight gradient's pixel-tile index (image-major, then tile rows, then tile columns)."""
    tr = 256 // p["twp"]
    ty = torch.arange(H).view(1, H, 1) // tr
    tx = torch.arange(W).view(1, 1, W) // p["twp"]
    return torch.arange(B).view(B, 1, 1) * (p["tiles_x"] * p["tiles_y"]) + ty * p["tiles_x"] + tx


def fault_halo_zero(c):
    """conv: the halo column left of the second column tile read as zero."""
    h, r, s = c.host, c.r, c.plan["twp"]
    assert c.plan["tiles_x"] == 2 and not r["transpose"]
    xm, wm = torch.zeros_like(h["x"]), torch.zeros_like(h["w"])
    xm[..., s - 1], wm[..., 0] = h["x"][..., s - 1], h["w"][..., 0]
    y0 = h["y0"].clone()
    y0[..., s] -= conv_ref(xm, wm, False)[..., s]
    return conv_expected(h, r, y0)


def fault_row_wrap(c):
    """conv: the right neighbour of a row's last pixel taken from the next row's first pixel instead of the zero padding."""
    h, r = c.host, c.r
    assert not r["transpose"] and r["H"] > 1
    xp = F.pad(h["x"].double(), (1, 1, 1, 1))
    xp[..., :-1, -1] = xp[..., 1:, 1]
    return conv_expected(h, r, F.conv2d(xp, h["w"].double()))


def fault_taps_swapped(c):
    """conv: taps 0 and 8 exchanged (a flip applied to, or missing from, the two corner taps)."""
    h, w = c.host, c.host["w"].clone()
    w[..., 0, 0], w[..., 2, 2] = h["w"][..., 2, 2], h["w"][..., 0, 0]
    return conv_expected(h, c.r, conv_ref(h["x"], w, c.r["transpose"]))


def fault_chunk_dropped(c):
    """conv: the last, partial 16-channel chunk never contracted."""
    h, r = c.host, c.r
    assert c.plan["chunks"] > 1 and r["K"] % 16 and not r["transpose"]
    x = h["x"].clone()
    x[:, 16 * (c.plan["chunks"] - 1):] = 0
    return conv_expected(h, r, conv_ref(x, h["w"], False))


def fault_split_dropped(c):
    """wgrad: the partial sum of split 1 left out of dw."""
    h, r, p = c.host, c.r, c.plan
    assert p["w_splits"] >= 2
    keep = (tile_of(p, r["B"], r["H"], r["W"]) % p["w_splits"] != 1).unsqueeze(1)
    return wgrad_ref(h["dy"] * keep, h["x"]) + (h["base"].double() if r["accumulate"] else 0)


def fault_phases_swapped(c):
    """pixel_shuffle2: the two column phases j exchanged."""
    r = c.r
    B, cc, H, W = r["B"], r["c"], r["H"], r["W"]
    ref = c.ref.view(B, cc, H, 2, W, 2) if not r["unshuffle"] else c.ref.view(B, cc, 2, 2, H, W)
    return ref.flip(5 if not r["unshuffle"] else 3).reshape(c.ref.shape)


def fault_band_seam(c):
    """im2col: the row above a band's first row (the halo of band 1 at band height 8) read as zero."""
    r = c.r
    assert r["form"] == "stream" and r["H"] > 8 and r["band"] == 8
    ref = c.ref.clone().view(r["B"], r["C"], 9, r["H"], r["W"])
    first = 6 if r["flip"] else 0                          # the three output planes that hold the row above (ky = 0 of the source tap)
    ref[:, :, first:first + 3, 8] = 0
    return ref.view(c.ref.shape)


def fault_bias_plane(c):
    """col2im: bias[plane] taken for bias[plane % M]."""
    r = c.r
    assert r["bias"] and r["B"] > 1
    bias = ints((r["C"],), 633, -8, 9).double()
    planes = torch.arange(r["B"] * r["C"])
    wrong = bias[(planes + planes // r["C"]) % r["C"]].view(r["B"], r["C"], 1, 1)          # another channel's bias from image 1 on
    return c.ref - bias.view(1, -1, 1, 1).to(c.ref.dtype) + wrong.to(c.ref.dtype)


FAULTS = {"halo_zero": ("conv", fault_halo_zero), "row_wrap": ("conv", fault_row_wrap), "taps_swapped": ("conv", fault_taps_swapped),
          "chunk_dropped": ("conv", fault_chunk_dropped), "split_dropped": ("wgrad", fault_split_dropped),
          "phases_swapped": ("shuffle", fault_phases_swapped), "band_seam": ("im2col", fault_band_seam),
          "bias_plane": ("col2im", fault_bias_plane)}


def fault_applies(name, r, p):
    return {"halo_zero": lambda: p["tiles_x"] == 2 and not r["transpose"],
            "row_wrap": lambda: not r["transpose"] and r["H"] > 1,
            "taps_swapped": lambda: r["H"] > 1,            # (on a one-row plane the corner taps see padding only)
            "chunk_dropped": lambda: p["chunks"] > 1 and r["K"] % 16 != 0 and not r["transpose"],
            "split_dropped": lambda: p["w_splits"] >= 2,
            "phases_swapped": lambda: r["trips"] == 1,
            "band_seam": lambda: r["form"] == "stream" and r["H"] > 8 and r["band"] == 8,
            "bias_plane": lambda: r["bias"] and r["B"] > 1 and not r["device_ref"]}[name]()

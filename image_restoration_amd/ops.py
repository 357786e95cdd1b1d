"""Tensor-level wrappers over the C-ABI (``include/mi_restore.h``).

PyTorch is plumbing here: it owns device memory (outputs, saved blobs and workspaces are torch
tensors, so the caching allocator and stream semantics apply) and supplies the current HIP stream.
All compute happens in ``libmi_restore.so``.  CPU tensors are rejected: there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L

Tensor = torch.Tensor


def _dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return L.MI_F32
    if dtype == torch.bfloat16:
        return L.MI_BF16
    raise TypeError(f"activations must be float32 or bfloat16, got {dtype}")


def _dt(t: Tensor) -> int:
    return _dtype_code(t.dtype)


def _gpu(*ts: Optional[Tensor]) -> None:
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("image_restoration_amd ops run on the MI355X only (got a CPU tensor); "
                               "the CPU restatement lives in oracle/ and is test infrastructure")
        if not t.is_contiguous():
            raise RuntimeError("image_restoration_amd ops need contiguous NCHW tensors")


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _f32(t: Optional[Tensor], what: str) -> Optional[Tensor]:
    if t is not None and t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (parameters and their gradients stay fp32), got {t.dtype}")
    return t


def _f32_struct(cls, ts: Sequence[Optional[Tensor]], what: str, *tail):
    """Struct ``cls`` of the pointers of ``ts`` (parameters or their gradients: each checked to be fp32), then ``tail``."""
    for t in ts:
        _f32(t, what)
    return cls(*[_p(t) for t in ts], *tail)


def _stream() -> int:
    # the raw handle of torch's current stream (torch.cuda.current_stream() builds a Stream object: 9 us per call)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _blob(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ----------------------------------------------------------------------------- A/B switches (environment variables)
# Read once per process (a TransformerBlock forward used to make eight os.environ look-ups); ``reload_env()`` re-reads them here
# and in the library (mi_env_reload) - for tests and A/B tools that flip a switch inside one process.
_ENV: dict = {}
_WEIGHTS_EPOCH = [0]


def env(name: str) -> Optional[str]:
    """Value of an MI_* switch as the process had it at first use / the last reload_env(); None when unset or empty."""
    try:
        return _ENV[name]
    except KeyError:
        v = os.environ.get(name) or None
        _ENV[name] = v
        return v


def reload_env() -> None:
    global _WS_CACHE_ON
    _ENV.clear()
    _WS_CACHE_ON = os.environ.get("MI_WS_CACHE", "1") != "0"
    if L._lib is not None:
        L.check(L.lib().mi_env_reload(), "env_reload")


def weights_epoch() -> int:
    """Counter of parameter updates torch cannot see (the fused AdamW kernel writes through raw pointers and bumps no version
    counter): every cache of data derived from the weights keys on it (restormer._fused_gdfn_pack, the fp8 scales)."""
    return _WEIGHTS_EPOCH[0]


def bump_weights_epoch() -> None:
    _WEIGHTS_EPOCH[0] += 1


_WS_CACHE: dict = {}
_WS_CACHE_ON = os.environ.get("MI_WS_CACHE", "1") != "0"


def _ws(nbytes: int, device) -> Tensor:
    """Scratch for ONE library call.  Calls are stream-ordered and a workspace is dead when its call returns, so one grow-only
    buffer per device serves them all (a launch-bound step made ~2000 allocator calls for these; MI_WS_CACHE=0: per-call blobs)."""
    n = max(int(nbytes), 256)
    if not _WS_CACHE_ON:
        return torch.empty(n, dtype=torch.uint8, device=device)
    key = device.index
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < n:
        buf = None
        _WS_CACHE.pop(key, None)                       # release the old one first
        buf = _WS_CACHE[key] = torch.empty(n, dtype=torch.uint8, device=device)
    return buf


# ----------------------------------------------------------------------------- what the module wrappers share
def _covered(sizer, shape) -> int:
    """Workspace bytes of ``shape``; a shape the kernels do not cover raises NotImplementedError with the library's reason."""
    ws_bytes = sizer(C.byref(shape))
    if ws_bytes == 0:
        raise NotImplementedError("image_restoration_amd: " + L.lib().mi_last_error().decode("utf-8", "replace"))
    return ws_bytes


def _sizes(saved_fn, ws_fn, shape) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) as the library's two sizing calls answer: (0, 0) for a shape the kernels do not cover."""
    return int(saved_fn(C.byref(shape))), int(ws_fn(C.byref(shape)))


def _out_saved_ws(x: Tensor, shape, saved_fn, need_saved: bool, ws_bytes: int):
    """What a module forward allocates: (out like x, the saved blob or None, the workspace)."""
    out = torch.empty_like(x)
    saved = _blob(saved_fn(C.byref(shape)), x.device) if need_saved else None
    return out, saved, _ws(ws_bytes, x.device)


def _out_ws(x: Tensor, ws_bytes: int):
    """What a module backward, or a forward that saves nothing, allocates: (dx / out like x, the workspace)."""
    return torch.empty_like(x), _ws(ws_bytes, x.device)


def _plan_report(fn, shape, who: str, keys: Sequence[str], first: int, sections: Sequence[str], saved=None,
                 tail: Sequence[str] = ("workspace", "saved_bytes")) -> dict:
    """Decodes the out[64] report of a module's mi_*_plan (the wire format: plan_report in csrc/internal.h): the scalars named by
    ``keys`` from slot 0, ``sections`` as (byte offset, bytes) pairs from slot ``first``, the saved blob's sections
    (``saved`` = (first slot, names)) where the module reports them, and the values from slot 60 on named by ``tail``."""
    out = (L.c_i64 * 64)()
    L.check(fn(C.byref(shape), out), who)
    return _decode_report(out, keys, first, sections, saved, tail, 60)


def _decode_report(out, keys, first, sections, saved, tail, tail_at) -> dict:
    def pairs(at, names):
        return {n: (int(out[at + 2 * i]), int(out[at + 2 * i + 1])) for i, n in enumerate(names)}
    plan = {k: int(out[i]) for i, k in enumerate(keys)}
    plan["sections"] = pairs(first, sections)
    if saved is not None:
        plan["saved_sections"] = pairs(*saved)
    plan.update((k, int(out[tail_at + i])) for i, k in enumerate(tail))
    return plan


# ----------------------------------------------------------------------------- LayerNorm
def ln_fwd(x: Tensor, w: Tensor, b: Optional[Tensor], with_bias: bool, want_stats: bool = True):
    _gpu(x, w, b)
    _f32(w, "LayerNorm weight"); _f32(b, "LayerNorm bias")
    B, Cc, H, W = x.shape
    y = torch.empty_like(x)
    mean = rstd = None
    if want_stats:
        mean = torch.empty((B, H * W), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
    L.check(L.lib().mi_ln_fwd(_p(x), _p(w), _p(b), _p(y), _p(mean), _p(rstd), B, Cc, H * W, int(with_bias), _dt(x),
                              _stream()), "ln_fwd")
    return y, mean, rstd


def ln_bwd(dy: Tensor, x: Tensor, w: Tensor, mean: Tensor, rstd: Tensor, dres: Optional[Tensor], with_bias: bool,
           dw: Tensor, db: Optional[Tensor], accumulate: bool) -> Tensor:
    _gpu(dy, x, w, mean, rstd, dres, dw, db)
    B, Cc, H, W = x.shape
    dx = torch.empty_like(x)
    ws = _ws(L.lib().mi_ln_bwd_workspace(B, Cc, H * W), x.device)
    L.check(L.lib().mi_ln_bwd(_p(dy), _p(x), _p(w), _p(mean), _p(rstd), _p(dres), _p(dx), _p(dw), _p(db), B, Cc, H * W,
                              int(with_bias), int(accumulate), _dt(x), _p(ws), _stream()), "ln_bwd")
    return dx


def ln_plan(B: int, C: int, N: int, dtype: torch.dtype, backward: bool, aligned: bool = True) -> dict:
    """What ln_fwd / ln_bwd launch for this call under the current MI_LN_FORM (mi_ln_plan; no GPU work).  aligned: every
    activation pointer is a multiple of 4 bytes.  rows / two_stage describe the backward's partial rows and their sum."""
    out = (L.C.c_int * 9)()   # (C is the channel count here)
    L.check(L.lib().mi_ln_plan(B, C, N, _dtype_code(dtype), int(backward), int(aligned), out), "ln_plan")
    tail = {"vec": out[4], "tiles": out[5], "gx": out[6], "rows": out[7], "two_stage": bool(out[8])}
    if out[0] == 1:
        return {"family": "wave", "CB": out[1], "WS": out[2], "NW": out[3], **tail}
    return {"family": "block", "waves": out[1], "CPT": out[2], **tail}


# ----------------------------------------------------------------------------- depthwise conv
def dwconv_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor]) -> Tensor:
    _gpu(x, w, bias)
    B, Cc, H, W = x.shape
    ks = w.shape[-1]
    y = torch.empty_like(x)
    L.check(L.lib().mi_dwconv_fwd(_p(x), _p(w), _p(bias), _p(y), B, Cc, H, W, ks, _dt(x), _stream()), "dwconv_fwd")
    return y


def dwconv_gate_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], want_y: bool = True):
    _gpu(x, w, bias)
    B, C2, H, W = x.shape
    ks = w.shape[-1]
    y = torch.empty_like(x) if want_y else None
    g = torch.empty((B, C2 // 2, H, W), dtype=x.dtype, device=x.device)
    L.check(L.lib().mi_dwconv_gate_fwd(_p(x), _p(w), _p(bias), _p(y), _p(g), B, C2, H, W, ks, _dt(x), _stream()),
            "dwconv_gate_fwd")
    return y, g


def dwconv_bwd(dy: Tensor, x: Tensor, w: Tensor, has_bias: bool, grads: Optional[Sequence[Optional[Tensor]]] = None):
    """grads = (dw, db) fp32 buffers to ACCUMULATE into (a trainer's main_grad slots); None: fresh tensors are returned."""
    _gpu(dy, x, w)
    B, Cc, H, W = x.shape
    ks = w.shape[-1]
    dx = torch.empty_like(x)
    acc = grads is not None
    dw = _f32(grads[0], "depthwise weight gradient") if acc else torch.empty_like(w)
    db = (_f32(grads[1], "depthwise bias gradient") if acc else torch.empty(Cc, dtype=torch.float32, device=x.device)) if has_bias else None
    ws = _ws(L.lib().mi_dwconv_bwd_workspace(B, Cc, H, W, ks), x.device)
    L.check(L.lib().mi_dwconv_bwd(_p(dy), _p(x), _p(w), _p(dx), _p(dw), _p(db), B, Cc, H, W, ks, 1 if acc else 0, _dt(x), _p(ws),
                                  _stream()), "dwconv_bwd")
    return dx, dw, db


def dwconv_gate_bwd(dg: Tensor, y: Tensor, x: Tensor, w: Tensor, has_bias: bool):
    _gpu(dg, y, x, w)
    B, C2, H, W = x.shape
    ks = w.shape[-1]
    dx = torch.empty_like(x)
    dw = torch.empty_like(w)
    db = torch.empty(C2, dtype=torch.float32, device=x.device) if has_bias else None
    ws = _ws(L.lib().mi_dwconv_bwd_workspace(B, C2, H, W, ks), x.device)
    L.check(L.lib().mi_dwconv_gate_bwd(_p(dg), _p(y), _p(x), _p(w), _p(dx), _p(dw), _p(db), B, C2, H, W, ks, 0, _dt(x),
                                       _p(ws), _stream()), "dwconv_gate_bwd")
    return dx, dw, db


# ----------------------------------------------------------------------------- pointwise GEMM / Gram
def dwconv_gate_recompute_ok(H: int, W: int, ks: int) -> bool:
    return bool(L.lib().mi_dwconv_gate_recompute_ok(H, W, ks))


DWCONV_PLAN_OPS = {"fwd": 0, "gate_fwd": 1, "bwd": 2, "gate_bwd": 3}


def dwconv_plan(B: int, C: int, H: int, W: int, ks: int, op: str) -> dict:
    """The launch plan the depthwise entry point `op` takes for 16-byte-aligned planes (mi_dwconv_plan; no GPU work)."""
    out = (L.C.c_int * 6)()   # (C is the channel count here)
    L.check(L.lib().mi_dwconv_plan(B, C, H, W, ks, DWCONV_PLAN_OPS[op], out), "dwconv_plan")
    if out[0] == 1:
        return {"family": "stream", "band": out[1], "nb": out[2], "lpr": out[3], "uni": bool(out[4]), "rows": out[5]}
    return {"family": "lds", "th": out[1], "bands": out[2], "tw": out[3], "uni": False, "rpt": out[5]}


def dwconv_gate_bwd_recompute(dg: Tensor, x: Tensor, w: Tensor, bias: Optional[Tensor]):
    """Gate backward with the conv outputs recomputed from the conv input x (no stored y)."""
    _gpu(dg, x, w, bias)
    B, C2, H, W = x.shape
    ks = w.shape[-1]
    dx = torch.empty_like(x)
    dw = torch.empty_like(w)
    db = torch.empty(C2, dtype=torch.float32, device=x.device) if bias is not None else None
    ws = _ws(L.lib().mi_dwconv_bwd_workspace(B, C2, H, W, ks), x.device)
    L.check(L.lib().mi_dwconv_gate_bwd_recompute(_p(dg), _p(x), _p(w), _p(bias), _p(dx), _p(dw), _p(db), B, C2, H, W, ks, 0,
                                                 _dt(x), _p(ws), _stream()), "dwconv_gate_bwd_recompute")
    return dx, dw, db


def conv1x1(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
            transposed: bool = False, x2: Optional[Tensor] = None, out: Optional[Tensor] = None,
            f8: Optional[Tuple[float, float]] = None) -> Tensor:
    """y = W x (+bias)(+residual).  x [B,K,H,W]; w [M,K(,1,1)] or, transposed, [K,M(,1,1)] used as W^T.
    x2: optional second K-panel (channel concat without the concat).  f8 = (sx, sw): fp8 e4m3 MFMA operands (x / sx, w / sw,
    powers of two; bf16 tensors, wave-owned kernel forms only - the call fails elsewhere)."""
    _gpu(x, w, bias, residual, x2)
    _f32(w, "1x1 weight"); _f32(bias, "1x1 bias")
    B, K1, H, W = x.shape
    K2 = 0 if x2 is None else x2.shape[1]
    N = H * W
    w2 = w.reshape(w.shape[0], -1)
    M = w2.shape[1] if transposed else w2.shape[0]
    assert (w2.shape[0] if transposed else w2.shape[1]) == K1 + K2, "weight/input channel mismatch"
    y = torch.empty((B, M, H, W), dtype=x.dtype, device=x.device) if out is None else out
    assert y.shape == (B, M, H, W) and y.is_contiguous() and y.dtype == x.dtype
    d = L.PwDesc()
    d.x1, d.x1_bs, d.x1_gs, d.k1 = _p(x), K1 * N, 0, K1
    d.x2, d.x2_bs, d.x2_gs, d.k2 = _p(x2), K2 * N, 0, K2
    d.w, d.w_bs, d.w_gs = _p(w2), 0, 0
    d.w_sm, d.w_sk = (1, w2.shape[1]) if transposed else (w2.shape[1], 1)
    d.bias, d.bias_gs = _p(bias), 0
    d.r, d.r_bs, d.r_gs = _p(residual), M * N, 0
    d.y, d.y_bs, d.y_gs = _p(y), M * N, 0
    d.m, d.n, d.batch, d.groups, d.dtype = M, N, B, 1, _dt(x)
    if f8 is not None:
        d.f8, d.f8_sx, d.f8_sw = 1, float(f8[0]), float(f8[1])
    pw_gemm_desc(d, x.device)
    return y


def pw_gemm_desc(d: "L.PwDesc", device) -> None:
    """Run one mi_pw_gemm call described by ``d`` (allocates its weight-pack workspace)."""
    ws = _ws(L.lib().mi_pw_gemm_workspace(C.byref(d)), device)
    L.check(L.lib().mi_pw_gemm(C.byref(d), _p(ws), _stream()), "pw_gemm")


PW_FAMILIES = ("chunked", "resident", "dma", "xres", "stream", "xwide", "lds")
PW_WEIGHTS = ("pack", "b16", "f32")
PW_PROBE = 256          # stands in for every pointer of a descriptor that is only planned: 16-byte aligned, never read


def pw_probe(M: int, K: int, N: int, dtype: torch.dtype, B: int = 1, groups: int = 1, K2: int = 0, per_image: bool = False,
             transposed: bool = False, residual: bool = False, misalign: int = 0) -> "L.PwDesc":
    """A dense descriptor of placeholder pointers for pw_plan and the mi_pw_gemm_*_ok / _workspace queries: x [B, groups*K, N]
    (+ a second panel of K2 channels), w [(B,) groups, M, K+K2] or its transpose, y (and residual) [B, groups*M, N].
    misalign: bytes added to the x / y / residual pointers."""
    d = L.PwDesc()
    kt = K + K2
    d.x1, d.x1_bs, d.x1_gs, d.k1 = PW_PROBE + misalign, groups * K * N, K * N, K
    if K2:
        d.x2, d.x2_bs, d.x2_gs, d.k2 = PW_PROBE, groups * K2 * N, K2 * N, K2
    d.w, d.w_bs, d.w_gs = PW_PROBE, (groups * M * kt if per_image else 0), (M * kt if groups > 1 else 0)
    d.w_sm, d.w_sk = (1, M) if transposed else (kt, 1)
    if residual:
        d.r = PW_PROBE + misalign
    d.r_bs, d.r_gs = groups * M * N, M * N
    d.y, d.y_bs, d.y_gs = PW_PROBE + misalign, groups * M * N, M * N
    d.m, d.n, d.batch, d.groups, d.dtype = M, N, B, groups, _dtype_code(dtype)
    return d


def pw_plan(d: "L.PwDesc") -> dict:
    """What mi_pw_gemm runs for ``d`` under the current MI_PW_* switches (mi_pw_plan; no GPU work)."""
    out = (L.c_i64 * 18)()
    L.check(L.lib().mi_pw_plan(C.byref(d), out), "pw_plan")
    return {"family": PW_FAMILIES[out[0]], "tm": out[1], "kb": out[2], "f8": bool(out[3]), "ln": bool(out[4]),
            "grid": (out[5], out[6], out[7]), "block": out[8], "lds": out[9], "tpw": out[10], "tpb": out[11], "n_slabs": out[12],
            "slabs_per": out[13], "xcd_map": bool(out[14]), "weights": PW_WEIGHTS[out[15]], "cacheable": bool(out[16]),
            "workspace": out[17]}


GRAM_FAMILIES = ("lds", "stream")
GRAM_FINISH = ("direct", "few4", "few16", "general")


def gram_probe(ma: int, mb: int, N: int, dtype: torch.dtype, B: int = 1, groups: int = 1, sum_batch: bool = False, sumsq: bool = False,
               accumulate: bool = False, out_ld: int = 0, misalign: int = 0) -> "L.GramDesc":
    """A dense descriptor of placeholder pointers for gram_plan and mi_gram_workspace: a [B, groups*ma, N], b [B, groups*mb, N],
    out [B*groups or groups, ma, mb] with row stride out_ld (0: mb).  misalign: bytes added to the a pointer."""
    d = L.GramDesc()
    d.a, d.a_bs, d.a_gs, d.ma = PW_PROBE + misalign, groups * ma * N, ma * N, ma
    d.b, d.b_bs, d.b_gs, d.mb = PW_PROBE, groups * mb * N, mb * N, mb
    d.n, d.batch, d.groups, d.dtype = N, B, groups, _dtype_code(dtype)
    d.sum_batch, d.accumulate = int(sum_batch), int(accumulate)
    d.out, d.out_ld, d.out_zs, d.sumsq = PW_PROBE, out_ld or mb, ma * mb, (PW_PROBE if sumsq else None)
    return d


def gram_desc(a: Tensor, b: Tensor, groups: int = 1, sum_batch: bool = False, want_sumsq: bool = False, out: Optional[Tensor] = None,
              accumulate: bool = False, ss: Optional[Tensor] = None) -> "L.GramDesc":
    """The descriptor ``gram`` runs for these operands.  out / ss not allocated yet keep the probe's placeholder: enough for
    gram_plan, which reads pointers for their alignment only."""
    B, Ca, H, W = a.shape
    d = gram_probe(Ca // groups, b.shape[1] // groups, H * W, a.dtype, B=B, groups=groups, sum_batch=sum_batch, sumsq=want_sumsq,
                   accumulate=accumulate)
    d.a, d.b = _p(a), _p(b)
    if out is not None:
        d.out = _p(out)
    if ss is not None:
        d.sumsq = _p(ss)
    return d


def gram_plan(d: "L.GramDesc") -> dict:
    """What mi_gram runs for ``d`` under the current MI_GRAM_* switches (mi_gram_plan; no GPU work)."""
    out = (L.c_i64 * 22)()
    L.check(L.lib().mi_gram_plan(C.byref(d), out), "gram_plan")
    return {"family": GRAM_FAMILIES[out[0]], "fa": out[1], "fb": out[2], "sumsq": bool(out[3]), "unit": out[4], "units": out[5],
            "per_split": out[6], "splits": out[7], "tiles_a": out[8], "tiles_b": out[9], "Z": out[10], "fold": out[11],
            "vec_ok": bool(out[12]), "grid": (out[13], out[14], out[15]), "block": out[16], "part_bytes": out[17], "ss_bytes": out[18],
            "finish": GRAM_FINISH[out[19]], "deferrable": bool(out[20]), "workspace": out[21]}


def gram(a: Tensor, b: Tensor, groups: int = 1, sum_batch: bool = False, want_sumsq: bool = False,
         out: Optional[Tensor] = None, accumulate: bool = False):
    """G[z][i][j] = sum_n a[z][i][n] b[z][j][n] with a,b [B, groups*m, H, W] split head-major into groups.
    out (+ accumulate): write / add the result into a caller's fp32 buffer of Z*ma*mb elements - a weight-gradient slot of the
    trainer's flat buffer; under the trainer's deferral window the final sum then joins the one table-driven reduction launch."""
    _gpu(a, b, out)
    B, Ca, H, W = a.shape
    ma, mb = Ca // groups, b.shape[1] // groups
    Z = groups if sum_batch else B * groups
    if out is None:
        if accumulate:
            raise ValueError("gram: accumulate needs the output buffer")
        out = torch.empty((Z, ma, mb), dtype=torch.float32, device=a.device)
    elif out.dtype != torch.float32 or out.numel() != Z * ma * mb:
        raise ValueError(f"gram: out must be float32 with {Z * ma * mb} elements")
    ss = torch.empty((B * groups, ma + mb), dtype=torch.float32, device=a.device) if want_sumsq else None
    d = gram_desc(a, b, groups, sum_batch, want_sumsq, out, accumulate, ss)
    ws = _ws(L.lib().mi_gram_workspace(C.byref(d)), a.device)
    L.check(L.lib().mi_gram(C.byref(d), _p(ws), _stream()), "gram")
    return (out, ss) if want_sumsq else out


def conv1x1_dgrad_panel(dy: Tensor, w2: Tensor, k0: int, k: int) -> Tensor:
    """dx[:, k0:k0+k] = W[:, k0:k0+k]^T dy  using the column block of w2 [M, K1+K2] in place (row stride stays K1+K2)."""
    B, M, H, W = dy.shape
    N = H * W
    dx = torch.empty((B, k, H, W), dtype=dy.dtype, device=dy.device)
    d = L.PwDesc()
    d.x1, d.x1_bs, d.k1 = _p(dy), M * N, M
    d.w = _p(w2) + 4 * k0
    d.w_sm, d.w_sk = 1, w2.shape[1]
    d.y, d.y_bs = _p(dx), k * N
    d.m, d.n, d.batch, d.groups, d.dtype = k, N, B, 1, _dt(dy)
    pw_gemm_desc(d, dy.device)
    return dx


def wgrad_panel_desc(dy: Tensor, xp: Tensor, dw2: Tensor, k0: int, accumulate: bool) -> "L.GramDesc":
    """The Gram of one K-panel: dy . xp^T summed over the batch into columns k0 .. of dw2 (row stride: dw2's full width)."""
    d = gram_desc(dy, xp, 1, True, accumulate=accumulate)
    d.out, d.out_ld = _p(dw2) + 4 * k0, dw2.shape[1]
    return d


def conv1x1_wgrad_panels(dy: Tensor, x1: Tensor, x2: Optional[Tensor], dw2: Tensor, accumulate: bool) -> None:
    """dw2[:, panel] (+)= dy . x^T for the K-panels x1, x2 of a 1x1 conv: each Gram lands in its column block of dw2 [M, K1+K2]."""
    B, M, H, W = dy.shape
    N = H * W
    k0 = 0
    for xp in (x1, x2):
        if xp is None:
            continue
        k = xp.shape[1]
        d = wgrad_panel_desc(dy, xp, dw2, k0, accumulate)
        ws = _blob(L.lib().mi_gram_workspace(C.byref(d)), dy.device)
        L.check(L.lib().mi_gram(C.byref(d), _p(ws), _stream()), "gram(wgrad panel)")
        k0 += k


# ----------------------------------------------------------------------------- MDTA / GDFN modules
MdtaParamsT = Tuple[Tensor, Tensor, Optional[Tensor], Tensor, Optional[Tensor], Tensor, Optional[Tensor]]
GdfnParamsT = Tuple[Tensor, Optional[Tensor], Tensor, Optional[Tensor], Tensor, Optional[Tensor]]


def _mdta_shape(x: Tensor, heads: int, ks: int) -> L.MdtaShape:
    B, Cc, H, W = x.shape
    return L.MdtaShape(B, Cc, heads, H, W, _dt(x), ks)


def _mdta_params(p: Sequence[Optional[Tensor]]) -> L.MdtaParams:
    return _f32_struct(L.MdtaParams, p, "MDTA parameter")


def mdta_saved_bytes(x: Tensor, heads: int, ks: int) -> int:
    """Size of the blob mdta_fwd saves for this activation (shape and dtype only: fake tensors do)."""
    return int(L.lib().mi_mdta_saved_bytes(C.byref(_mdta_shape(x, heads, ks))))


LnHeadT = Tuple[Tensor, Optional[Tensor], bool]     # LayerNorm weight, bias, want_stats


def _ln_head(ln: LnHeadT, x: Tensor):
    w, b, want_stats = ln
    _gpu(w, b)
    _f32(w, "LayerNorm weight"); _f32(b, "LayerNorm bias")
    mean = rstd = None
    if want_stats:
        mean = torch.empty((x.shape[0], x.shape[2] * x.shape[3]), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
    return L.LnHead(_p(w), _p(b), _p(mean), _p(rstd), int(b is not None)), mean, rstd


def mdta_fwd_ln_ok(x: Tensor, heads: int, ks: int) -> bool:
    """Can norm1 run inside the qkv GEMM (mi_mdta_fwd_ln)?"""
    if not x.is_cuda:
        return False
    s = _mdta_shape(x, heads, ks)
    return bool(L.lib().mi_mdta_fwd_ln_ok(C.byref(s)))


F8ScalesT = Tuple[float, float, float, float]       # x1, w1 (first projection: input, weight), x2, w2 (second projection)


def mdta_fwd_f8_ok(x: Tensor, heads: int, ks: int, with_ln: bool) -> bool:
    """Can both MDTA projections run on fp8 MFMA operands (mi_mdta_fwd_f8)?"""
    if not x.is_cuda or x.dtype != torch.bfloat16:
        return False
    s = _mdta_shape(x, heads, ks)
    return bool(L.lib().mi_mdta_fwd_f8_ok(C.byref(s), int(with_ln)))


def mdta_fwd(x: Tensor, residual: Optional[Tensor], params: MdtaParamsT, heads: int, need_saved: bool,
             ln: Optional[LnHeadT] = None, f8: Optional[F8ScalesT] = None):
    """params = (temperature, qkv.weight, qkv.bias, qkv_dwconv.weight, qkv_dwconv.bias, project_out.weight, .bias).
    ln = (weight, bias, want_stats): x is the LayerNorm INPUT and the norm runs inside the qkv GEMM; returns
    (out, saved, mean, rstd) then.  f8 = (x1, w1, x2, w2): inference with fp8 e4m3 MFMA operands in both projections
    (nothing saved, no statistics); returns out."""
    _gpu(x, residual, *params)
    ks = params[3].shape[-1]
    s = _mdta_shape(x, heads, ks)
    lib = L.lib()
    out = torch.empty_like(x)
    if f8 is not None:
        if need_saved or (ln is not None and ln[2]):
            raise ValueError("fp8 projections are an inference path: nothing can be saved")
        ws = _ws(lib.mi_mdta_workspace(C.byref(s)), x.device)
        lh = _ln_head(ln, x)[0] if ln is not None else None
        L.check(lib.mi_mdta_fwd_f8(C.byref(s), C.byref(_mdta_params(params)), C.byref(lh) if lh is not None else None,
                                   C.byref(L.F8Scales(*[float(v) for v in f8])), _p(x), _p(residual), _p(out), _p(ws),
                                   _stream()), "mdta_fwd_f8")
        return out
    saved = _blob(lib.mi_mdta_saved_bytes(C.byref(s)), x.device) if need_saved else None
    ws = _ws(lib.mi_mdta_workspace(C.byref(s)), x.device)
    pp = _mdta_params(params)
    if ln is None:
        L.check(lib.mi_mdta_fwd(C.byref(s), C.byref(pp), _p(x), _p(residual), _p(out), _p(saved), _p(ws), _stream()),
                "mdta_fwd")
        return out, saved
    lh, mean, rstd = _ln_head(ln, x)
    L.check(lib.mi_mdta_fwd_ln(C.byref(s), C.byref(pp), C.byref(lh), _p(x), _p(residual), _p(out), _p(saved), _p(ws),
                               _stream()), "mdta_fwd_ln")
    return out, saved, mean, rstd


LnTailT = Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor], Tensor, Tensor]   # w, b, mean, rstd, dres, dw, db


def _ln_tail(ln: LnTailT, like: Tensor) -> L.LnTail:
    w, b, mean, rstd, dres, dw, db = ln
    _gpu(w, b, mean, rstd, dres, dw, db)
    for t_ in (w, b, mean, rstd, dw, db):
        _f32(t_, "LayerNorm tail tensor")
    if dres is not None and (dres.shape != like.shape or dres.dtype != like.dtype):
        raise ValueError("LayerNorm tail: dres must match the block input")
    return L.LnTail(_p(w), _p(b), _p(mean), _p(rstd), _p(dres), _p(dw), _p(db))


def mdta_bwd_ln_ok(x: Tensor, heads: int, ks: int, qkv_bias: bool) -> bool:
    """Can the MDTA backward end in the one-launch tail (qkv weight gradient + W^T dY + LayerNorm backward + residual)?"""
    if not x.is_cuda:
        return False
    s = _mdta_shape(x, heads, ks)
    return bool(L.lib().mi_mdta_bwd_ln_ok(C.byref(s), int(qkv_bias)))


def mdta_bwd(x: Tensor, dout: Tensor, params: MdtaParamsT, heads: int, saved: Tensor,
             grads: Sequence[Optional[Tensor]], accumulate: bool, ln: Optional[LnTailT] = None) -> Tensor:
    """ln = None: x is the LayerNorm output (the conv input), the result its gradient.  ln given: x is the LayerNorm INPUT
    and the result the gradient of the half-block's input (mi_mdta_bwd_ln)."""
    _gpu(x, dout, saved, *params, *grads)
    ks = params[3].shape[-1]
    s = _mdta_shape(x, heads, ks)
    lib = L.lib()
    dx = torch.empty_like(x)
    pp = _mdta_params(params)
    gg = _f32_struct(L.MdtaGrads, grads, "MDTA gradient", int(accumulate))
    if ln is None:
        ws = _ws(lib.mi_mdta_workspace(C.byref(s)), x.device)
        L.check(lib.mi_mdta_bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()),
                "mdta_bwd")
    else:
        lt = _ln_tail(ln, x)
        ws = _ws(lib.mi_mdta_bwd_ln_workspace(C.byref(s)), x.device)
        L.check(lib.mi_mdta_bwd_ln(C.byref(s), C.byref(pp), C.byref(lt), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved),
                                   _p(ws), _stream()), "mdta_bwd_ln")
    return dx


def _xmdta_shape(x: Tensor, heads: int, ks_q: int, ks_kv: int) -> L.XmdtaShape:
    B, Cc, H, W = x.shape
    return L.XmdtaShape(B, Cc, heads, H, W, _dt(x), ks_q, ks_kv)


def xmdta_fwd(x: Tensor, y: Tensor, residual: Optional[Tensor], params: Sequence[Optional[Tensor]], heads: int,
              need_saved: bool):
    """Cross-MDTA.  params = (temperature, q.weight, q.bias, q_dwconv.weight, q_dwconv.bias, kv.weight, kv.bias,
    kv_dwconv.weight, kv_dwconv.bias, project_out.weight, project_out.bias)."""
    _gpu(x, y, residual, *params)
    assert x.shape == y.shape and x.dtype == y.dtype, "cross-MDTA needs x and y of one shape and dtype"
    s = _xmdta_shape(x, heads, params[3].shape[-1], params[7].shape[-1])
    lib = L.lib()
    out = torch.empty_like(x)
    saved = _blob(lib.mi_xmdta_saved_bytes(C.byref(s)), x.device) if need_saved else None
    ws = _ws(lib.mi_xmdta_workspace(C.byref(s)), x.device)
    pp = _f32_struct(L.XmdtaParams, params, "cross-MDTA parameter")
    L.check(lib.mi_xmdta_fwd(C.byref(s), C.byref(pp), _p(x), _p(y), _p(residual), _p(out), _p(saved), _p(ws), _stream()),
            "xmdta_fwd")
    return out, saved


def xmdta_bwd(x: Tensor, y: Tensor, dout: Tensor, params: Sequence[Optional[Tensor]], heads: int, saved: Tensor,
              grads: Sequence[Optional[Tensor]], accumulate: bool):
    _gpu(x, y, dout, saved, *params, *grads)
    s = _xmdta_shape(x, heads, params[3].shape[-1], params[7].shape[-1])
    lib = L.lib()
    dx, dy = torch.empty_like(x), torch.empty_like(y)
    ws = _ws(lib.mi_xmdta_workspace(C.byref(s)), x.device)
    pp = _f32_struct(L.XmdtaParams, params, "cross-MDTA parameter")
    gg = _f32_struct(L.XmdtaGrads, grads, "cross-MDTA gradient", int(accumulate))
    L.check(lib.mi_xmdta_bwd(C.byref(s), C.byref(pp), _p(x), _p(y), _p(dout), _p(dx), _p(dy), C.byref(gg), _p(saved), _p(ws),
                             _stream()), "xmdta_bwd")
    return dx, dy


def _gdfn_shape(x: Tensor, hidden: int, ks: int, flags: int = 0) -> L.GdfnShape:
    B, Cc, H, W = x.shape
    return L.GdfnShape(B, Cc, hidden, H, W, _dt(x), ks, flags)


def _gdfn_train_shape(x: Tensor, hidden: int, ks: int) -> L.GdfnShape:
    """The shape a training forward carves its blob for.  A/B switch MI_GDFN_STORE_Y: keep the conv output instead of
    recomputing it in backward.  Read here, once per forward; backward recovers the choice from the blob's size, so toggling
    the variable between the two cannot desynchronise them."""
    return _gdfn_shape(x, hidden, ks, 1 if env("MI_GDFN_STORE_Y") else 0)


def gdfn_saved_bytes(x: Tensor, hidden: int, ks: int) -> int:
    """Size of the blob gdfn_fwd saves for this activation (shape and dtype only: fake tensors do)."""
    return int(L.lib().mi_gdfn_saved_bytes(C.byref(_gdfn_train_shape(x, hidden, ks))))


def _gdfn_params(p: Sequence[Optional[Tensor]]) -> L.GdfnParams:
    return _f32_struct(L.GdfnParams, p, "GDFN parameter")


def gdfn_fwd_ln_ok(x: Tensor, hidden: int, ks: int) -> bool:
    if not x.is_cuda:
        return False
    s = _gdfn_shape(x, hidden, ks, 0)
    return bool(L.lib().mi_gdfn_fwd_ln_ok(C.byref(s)))


def gdfn_fwd_f8_ok(x: Tensor, hidden: int, ks: int, with_ln: bool) -> bool:
    if not x.is_cuda or x.dtype != torch.bfloat16:
        return False
    s = _gdfn_shape(x, hidden, ks, 0)
    return bool(L.lib().mi_gdfn_fwd_f8_ok(C.byref(s), int(with_ln)))


def gdfn_fwd(x: Tensor, residual: Optional[Tensor], params: GdfnParamsT, need_saved: bool, ln: Optional[LnHeadT] = None,
             f8: Optional[F8ScalesT] = None):
    """params = (project_in.weight, .bias, dwconv.weight, .bias, project_out.weight, .bias).  ln, f8: as in mdta_fwd."""
    _gpu(x, residual, *params)
    hidden, ks = params[4].shape[1], params[2].shape[-1]
    pp = _gdfn_params(params)
    if f8 is not None:
        if need_saved or (ln is not None and ln[2]):
            raise ValueError("fp8 projections are an inference path: nothing can be saved")
        s = _gdfn_shape(x, hidden, ks, 0)
        lib = L.lib()
        out = torch.empty_like(x)
        ws = _ws(lib.mi_gdfn_workspace(C.byref(s)), x.device)
        lh = _ln_head(ln, x)[0] if ln is not None else None
        L.check(lib.mi_gdfn_fwd_f8(C.byref(s), C.byref(pp),
                                   C.byref(lh) if lh is not None else None, C.byref(L.F8Scales(*[float(v) for v in f8])),
                                   _p(x), _p(residual), _p(out), _p(ws), _stream()), "gdfn_fwd_f8")
        return out
    s = _gdfn_train_shape(x, hidden, ks)
    lib = L.lib()
    out = torch.empty_like(x)
    saved = _blob(lib.mi_gdfn_saved_bytes(C.byref(s)), x.device) if need_saved else None
    ws = _ws(lib.mi_gdfn_workspace(C.byref(s)), x.device)
    if ln is None:
        L.check(lib.mi_gdfn_fwd(C.byref(s), C.byref(pp), _p(x), _p(residual), _p(out), _p(saved), _p(ws), _stream()),
                "gdfn_fwd")
        return out, saved
    lh, mean, rstd = _ln_head(ln, x)
    L.check(lib.mi_gdfn_fwd_ln(C.byref(s), C.byref(pp), C.byref(lh), _p(x), _p(residual), _p(out), _p(saved), _p(ws),
                               _stream()), "gdfn_fwd_ln")
    return out, saved, mean, rstd


def gdfn_bwd_ln_ok(x: Tensor, hidden: int, ks: int, in_bias: bool) -> bool:
    if not x.is_cuda:
        return False
    s = _gdfn_shape(x, hidden, ks, 0)
    return bool(L.lib().mi_gdfn_bwd_ln_ok(C.byref(s), int(in_bias)))


def gdfn_bwd(x: Tensor, dout: Tensor, params: GdfnParamsT, saved: Tensor, grads: Sequence[Optional[Tensor]],
             accumulate: bool, ln: Optional[LnTailT] = None) -> Tensor:
    """ln: as in mdta_bwd (x is then the LayerNorm INPUT; mi_gdfn_bwd_ln)."""
    _gpu(x, dout, saved, *params, *grads)
    hidden, ks = params[4].shape[1], params[2].shape[-1]
    lib = L.lib()
    s = None
    for flags in (0, 1):                   # which layout did the forward carve?  the two differ in size
        cand = _gdfn_shape(x, hidden, ks, flags)
        if max(int(lib.mi_gdfn_saved_bytes(C.byref(cand))), 256) == saved.numel():
            s = cand
            break
    if s is None:
        raise RuntimeError("gdfn_bwd: the saved blob matches neither layout of this shape")
    dx = torch.empty_like(x)
    pp = _gdfn_params(params)
    gg = _f32_struct(L.GdfnGrads, grads, "GDFN gradient", int(accumulate))
    if ln is None:
        ws = _ws(lib.mi_gdfn_workspace(C.byref(s)), x.device)
        L.check(lib.mi_gdfn_bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()),
                "gdfn_bwd")
    else:
        lt = _ln_tail(ln, x)
        ws = _ws(lib.mi_gdfn_bwd_ln_workspace(C.byref(s)), x.device)
        L.check(lib.mi_gdfn_bwd_ln(C.byref(s), C.byref(pp), C.byref(lt), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved),
                                   _p(ws), _stream()), "gdfn_bwd_ln")
    return dx


# ----------------------------------------------------------------------------- DRSformer: TKSA / MSFN
def tksa_topk(c: int) -> Tuple[int, int, int, int]:
    """The four top-k sizes of DRSformer_arch.py:141-155, with the reference's own expressions."""
    return int(c / 2), int(c * 2 / 3), int(c * 3 / 4), int(c * 4 / 5)


def _tksa_shape(x: Tensor, heads: int, topk: Sequence[int]) -> L.TksaShape:
    B, Cc, H, W = x.shape
    return L.TksaShape(B, Cc, heads, H, W, _dt(x), *[int(k) for k in topk])


def tksa_sizes(B: int, Cc: int, heads: int, H: int, W: int, dtype: torch.dtype, topk: Sequence[int]) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one TKSA call; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = L.TksaShape(B, Cc, heads, H, W, _dtype_code(dtype), *[int(k) for k in topk])
    return _sizes(L.lib().mi_tksa_saved_bytes, L.lib().mi_tksa_workspace, s)


def tksa_fwd(x: Tensor, residual: Optional[Tensor], params: Sequence[Optional[Tensor]], heads: int, topk: Sequence[int],
             need_saved: bool, want_scores: bool = False):
    """DRSformer Attention (TKSA).  params = (temperature, qkv.weight, qkv.bias, qkv_dwconv.weight, qkv_dwconv.bias,
    project_out.weight, project_out.bias, attn1, attn2, attn3, attn4); topk: the four k (tksa_topk).  Returns (out, saved) or,
    with want_scores, (out, saved, scores [B, heads, c, c] fp32: the S the top-k masks were ranked from)."""
    _gpu(x, residual, *params)
    s = _tksa_shape(x, heads, topk)
    lib = L.lib()
    ws_bytes = lib.mi_tksa_workspace(C.byref(s))
    if ws_bytes == 0:
        L.check(-1, "tksa_workspace")
    out, saved, ws = _out_saved_ws(x, s, lib.mi_tksa_saved_bytes, need_saved, ws_bytes)
    c = x.shape[1] // heads
    scores = torch.empty((x.shape[0], heads, c, c), dtype=torch.float32, device=x.device) if want_scores else None
    pp = _mdta_params(params[:7])
    tp = _f32_struct(L.TksaParams, params[7:11], "TKSA parameter")
    L.check(lib.mi_tksa_fwd(C.byref(s), C.byref(pp), C.byref(tp), _p(x), _p(residual), _p(out), _p(saved), _p(ws), _p(scores),
                            _stream()), "tksa_fwd")
    return (out, saved, scores) if want_scores else (out, saved)


def tksa_bwd(x: Tensor, dout: Tensor, params: Sequence[Optional[Tensor]], heads: int, topk: Sequence[int], saved: Tensor,
             grads: Sequence[Optional[Tensor]], accumulate: bool) -> Tensor:
    """Backward of tksa_fwd: dx; the 11 parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(x, dout, saved, *params, *grads)
    s = _tksa_shape(x, heads, topk)
    lib = L.lib()
    dx, ws = _out_ws(x, lib.mi_tksa_workspace(C.byref(s)))
    pp = _mdta_params(params[:7])
    tp = _f32_struct(L.TksaParams, params[7:11], "TKSA parameter")
    gg = _f32_struct(L.MdtaGrads, grads[:7], "TKSA gradient", int(accumulate))
    tg = _f32_struct(L.TksaGrads, grads[7:11], "TKSA gradient")
    L.check(lib.mi_tksa_bwd(C.byref(s), C.byref(pp), C.byref(tp), _p(x), _p(dout), _p(dx), C.byref(gg), C.byref(tg), _p(saved),
                            _p(ws), _stream()), "tksa_bwd")
    return dx


def _msfn_shape(x: Tensor, hidden: int) -> L.MsfnShape:
    B, Cc, H, W = x.shape
    return L.MsfnShape(B, Cc, hidden, H, W, _dt(x))


def msfn_fwd(x: Tensor, residual: Optional[Tensor], params: Sequence[Optional[Tensor]], need_saved: bool):
    """DRSformer FeedForward (MSFN).  params = (project_in.weight, .bias, dwconv3x3.weight, .bias, dwconv5x5.weight, .bias,
    dwconv3x3_1.weight, .bias, dwconv5x5_1.weight, .bias, project_out.weight, .bias).  Returns (out, saved)."""
    _gpu(x, residual, *params)
    s = _msfn_shape(x, params[6].shape[0])
    lib = L.lib()
    out, saved, ws = _out_saved_ws(x, s, lib.mi_msfn_saved_bytes, need_saved, lib.mi_msfn_workspace(C.byref(s)))
    pp = _f32_struct(L.MsfnParams, params, "MSFN parameter")
    L.check(lib.mi_msfn_fwd(C.byref(s), C.byref(pp), _p(x), _p(residual), _p(out), _p(saved), _p(ws), _stream()), "msfn_fwd")
    return out, saved


def msfn_saved_views(saved: Tensor, x: Tensor, hidden: int) -> dict:
    """The planes a training forward keeps in its saved blob: h0 (project_in output), a, b (stage-1 outputs) and y
    (cat(y1, y2)), each [B, 2h, H, W] in x's dtype - views into the blob (mi_msfn_saved_bytes' layout)."""
    B, _, H, W = x.shape
    n = B * 2 * hidden * H * W
    es = x.element_size()
    step = (n * es + 255) // 256 * 256
    return {name: saved[i * step:i * step + n * es].view(x.dtype).view(B, 2 * hidden, H, W)
            for i, name in enumerate(("h0", "a", "b", "y"))}


def msfn_bwd(x: Tensor, dout: Tensor, params: Sequence[Optional[Tensor]], saved: Tensor, grads: Sequence[Optional[Tensor]],
             accumulate: bool) -> Tensor:
    _gpu(x, dout, saved, *params, *grads)
    s = _msfn_shape(x, params[6].shape[0])
    lib = L.lib()
    dx, ws = _out_ws(x, lib.mi_msfn_workspace(C.byref(s)))
    pp = _f32_struct(L.MsfnParams, params, "MSFN parameter")
    gg = _f32_struct(L.MsfnGrads, grads, "MSFN gradient", int(accumulate))
    L.check(lib.mi_msfn_bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()),
            "msfn_bwd")
    return dx


# ----------------------------------------------------------------------------- DarkIR: dilated gate, pair conv, DBlock
DILGATE_MAX_BRANCHES, DILGATE_MAX_DILATION = 4, 16


def ln_fwd_eps(x: Tensor, w: Tensor, b: Optional[Tensor], with_bias: bool, eps: float, want_stats: bool = True):
    """ln_fwd with the caller's eps (DarkIR's LayerNorm2d: 1e-6).  -> (y, mean, rstd)."""
    _gpu(x, w, b)
    _f32(w, "LayerNorm weight"); _f32(b, "LayerNorm bias")
    B, Cc, H, W = x.shape
    y = torch.empty_like(x)
    mean = rstd = None
    if want_stats:
        mean = torch.empty((B, H * W), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
    L.check(L.lib().mi_ln_fwd_eps(_p(x), _p(w), _p(b), _p(y), _p(mean), _p(rstd), B, Cc, H * W, int(with_bias), float(eps), _dt(x),
                                  _stream()), "ln_fwd_eps")
    return y, mean, rstd


def _dil_array(dilations: Sequence[int]):
    return (C.c_int * max(len(dilations), 1))(*[int(d) for d in dilations])


def dilgate_plan(B: int, c: int, H: int, W: int, dtype: torch.dtype, dilations: Sequence[int]) -> dict:
    """What dilgate_fwd / dilgate_bwd launch for x [B, 2c, H, W] (mi_dilgate_plan; no GPU work)."""
    out = (L.c_i64 * 12)()
    L.check(L.lib().mi_dilgate_plan(B, c, H, W, _dtype_code(dtype), len(dilations), _dil_array(dilations), out), "dilgate_plan")
    names = ("tile_rows", "tile_cols", "halo", "lds_bytes", "grid_x", "grid_y", "grid_z", "pool_partials", "z_stored", "fwd_ws_bytes",
             "bwd_splits", "bwd_ws_bytes")
    plan = {n: int(v) for n, v in zip(names, out)}
    plan["z_stored"] = bool(plan["z_stored"])
    return plan


def _table_struct(fields, cls, ts: Sequence[Optional[Tensor]], n_dil: int, what: str, *tail):
    """Struct ``cls`` (parameters, or their gradients with ``accumulate`` as ``tail``) from the flat list ``ts`` over a field table
    like L.DBLOCK_FIELDS: (name, 1) takes one tensor, (name, 4) one per branch (n_dil of them).  Each is checked to be fp32."""
    for t in ts:
        _f32(t, what)
    st = cls()
    it = iter(ts)
    for name, k in fields:
        if k == 1:
            setattr(st, name, _p(next(it)))
        else:
            arr = getattr(st, name)
            for i in range(n_dil):
                arr[i] = _p(next(it))
    if tail:
        st.accumulate = tail[0]
    return st


def _dilgate_struct(cls, ws_: Sequence[Tensor], bs: Sequence[Optional[Tensor]], what: str, *tail):
    n = min(len(ws_), len(bs))
    return _table_struct((("w", 4), ("b", 4)), cls, (*ws_[:n], *bs[:n]), n, what, *tail)


def dilgate_fwd(x: Tensor, weights: Sequence[Tensor], biases: Sequence[Optional[Tensor]], dilations: Sequence[int]):
    """Sum of the dilated depthwise 3x3 convs (weights[i] [2c,1,3,3], biases[i] [2c] or None, dilation dilations[i]) on x
    [B, 2c, H, W], SimpleGate and the pool sums.  -> (g [B, c, H, W], pool [B, c] fp32 = sum over the plane of g)."""
    _gpu(x, *weights, *biases)
    B, C2, H, W = x.shape
    c = C2 // 2
    lib = L.lib()
    g = torch.empty((B, c, H, W), dtype=x.dtype, device=x.device)
    pool = torch.empty((B, c), dtype=torch.float32, device=x.device)
    ws = _ws(lib.mi_dilgate_fwd_workspace(B, c, H, W), x.device)
    pp = _dilgate_struct(L.DilgateParams, weights, biases, "dilgate parameter")
    L.check(lib.mi_dilgate_fwd(_p(x), C.byref(pp), _p(g), _p(pool), B, c, H, W, len(dilations), _dil_array(dilations), _dt(x), _p(ws),
                               _stream()), "dilgate_fwd")
    return g, pool


def dilgate_bwd(dg: Tensor, dg_add: Optional[Tensor], x: Tensor, weights: Sequence[Tensor], biases: Sequence[Optional[Tensor]],
                dilations: Sequence[int], gw: Sequence[Tensor], gb: Sequence[Optional[Tensor]], accumulate: bool) -> Tensor:
    """Backward of dilgate_fwd: dx; the weight / bias gradients of every branch are written (accumulate: added) into gw / gb.
    dg_add [B, c] fp32 or None: added to every pixel of dg's plane (the gradient through the pooled mean)."""
    _gpu(dg, dg_add, x, *weights, *biases, *gw, *gb)
    _f32(dg_add, "dg_add")
    B, C2, H, W = x.shape
    c = C2 // 2
    lib = L.lib()
    dx = torch.empty_like(x)
    ws = _ws(lib.mi_dilgate_bwd_workspace(B, c, H, W, len(dilations), _dt(x)), x.device)
    pp = _dilgate_struct(L.DilgateParams, weights, biases, "dilgate parameter")
    gg = _dilgate_struct(L.DilgateGrads, gw, gb, "dilgate gradient", int(accumulate))
    L.check(lib.mi_dilgate_bwd(_p(dg), _p(dg_add), _p(x), C.byref(pp), _p(dx), C.byref(gg), B, c, H, W, len(dilations),
                               _dil_array(dilations), _dt(x), _p(ws), _stream()), "dilgate_bwd")
    return dx


def pairconv3x3_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor]) -> Tensor:
    """3x3 conv, padding 1, on 2c channels in c groups (w [2c,2,3,3]): DarkIR's extra_conv."""
    _gpu(x, w, bias)
    _f32(w, "pairconv3x3 weight"); _f32(bias, "pairconv3x3 bias")
    B, C2, H, W = x.shape
    y = torch.empty_like(x)
    L.check(L.lib().mi_pairconv3x3_fwd(_p(x), _p(w), _p(bias), _p(y), B, C2 // 2, H, W, _dt(x), _stream()), "pairconv3x3_fwd")
    return y


def pairconv3x3_bwd(dy: Tensor, x: Tensor, w: Tensor, dw: Tensor, db: Optional[Tensor], accumulate: bool) -> Tensor:
    _gpu(dy, x, w, dw, db)
    _f32(w, "pairconv3x3 weight"); _f32(dw, "pairconv3x3 gradient"); _f32(db, "pairconv3x3 gradient")
    B, C2, H, W = x.shape
    lib = L.lib()
    dx = torch.empty_like(x)
    ws = _ws(lib.mi_pairconv3x3_bwd_workspace(B, C2 // 2, H, W), x.device)
    L.check(lib.mi_pairconv3x3_bwd(_p(dy), _p(x), _p(w), _p(dx), _p(dw), _p(db), B, C2 // 2, H, W, int(accumulate), _dt(x), _p(ws),
                                   _stream()), "pairconv3x3_bwd")
    return dx


def _block_shape(cls, B: int, Cc: int, H: int, W: int, dtype_code: int, dilations: Sequence[int], extra: bool):
    """mi_dblock_shape / mi_eblock_shape (``cls``: L.DblockShape / L.EblockShape; the same fields)."""
    s = cls(B, Cc, H, W, dtype_code, len(dilations))
    for i, d in enumerate(dilations[:4]):
        s.dil[i] = int(d)
    s.extra = int(extra)
    return s


_dblock_shape = functools.partial(_block_shape, L.DblockShape)


def dblock_sizes(B: int, Cc: int, H: int, W: int, dtype: torch.dtype, dilations: Sequence[int], extra: bool) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one DBlock; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = _dblock_shape(B, Cc, H, W, _dtype_code(dtype), dilations, extra)
    return _sizes(L.lib().mi_dblock_saved_bytes, L.lib().mi_dblock_workspace, s)


# mi_dblock_params / mi_dblock_grads from the flat list: norm1 (2), conv1 (2), extra_conv (2, None without it), the branches'
# weights (n_dil), their biases (n_dil), sca (2), conv3 (2), beta, norm2 (2), conv4 (2), conv5 (2), gamma
_dblock_struct = functools.partial(_table_struct, L.DBLOCK_FIELDS)


def dblock_fwd(x: Tensor, params: Sequence[Optional[Tensor]], dilations: Sequence[int], extra: bool, need_saved: bool):
    """DarkIR DBlock.forward.  params: see _dblock_struct.  -> (out, saved)."""
    _gpu(x, *params)
    B, Cc, H, W = x.shape
    s = _dblock_shape(B, Cc, H, W, _dt(x), dilations, extra)
    lib = L.lib()
    ws_bytes = lib.mi_dblock_workspace(C.byref(s))
    if ws_bytes == 0:
        L.check(-1, "dblock_workspace")
    out, saved, ws = _out_saved_ws(x, s, lib.mi_dblock_saved_bytes, need_saved, ws_bytes)
    pp = _dblock_struct(L.DblockParams, params, len(dilations), "DBlock parameter")
    L.check(lib.mi_dblock_fwd(C.byref(s), C.byref(pp), _p(x), _p(out), _p(saved), _p(ws), _stream()), "dblock_fwd")
    return out, saved


def dblock_bwd(x: Tensor, dout: Tensor, params: Sequence[Optional[Tensor]], dilations: Sequence[int], extra: bool, saved: Tensor,
               grads: Sequence[Optional[Tensor]], accumulate: bool) -> Tensor:
    """Backward of dblock_fwd: dx; the parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(x, dout, saved, *params, *grads)
    B, Cc, H, W = x.shape
    s = _dblock_shape(B, Cc, H, W, _dt(x), dilations, extra)
    lib = L.lib()
    dx, ws = _out_ws(x, lib.mi_dblock_workspace(C.byref(s)))
    pp = _dblock_struct(L.DblockParams, params, len(dilations), "DBlock parameter")
    gg = _dblock_struct(L.DblockGrads, grads, len(dilations), "DBlock gradient", int(accumulate))
    L.check(lib.mi_dblock_bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()), "dblock_bwd")
    return dx


# ----------------------------------------------------------------------------- DarkIR: FreMLP and the real 2-D transforms
FREMLP_MAX_HW, FREMLP_MAX_NC, FREMLP_MAX_HIDDEN = 512, 256, 512
_FREMLP_PLAN_KEYS = ("planes", "K", "hidden", "tile_m", "tile_k", "l_block", "l_blocks", "x_block", "x_blocks", "m_tiles_folded",
                     "m_tiles_plane", "grid_tables", "grid_rows_k", "grid_planes", "grid_rows_w", "grid_bins", "grid_hidden", "block",
                     "kernels_fwd", "kernels_bwd", "lib_calls_fwd", "lib_calls_bwd")
_FREMLP_SECTIONS = ("cos_w", "sin_w", "cos_wt", "sin_wt", "wcos_w", "wsin_w", "wcos_wt", "wsin_wt", "cos_h", "sin_h", "T", "U", "Z",
                    "hidden", "m1", "m2", "pw_ws", "gram_ws", "chan_sum_ws")
_FREMLP_PLAN = dict(keys=_FREMLP_PLAN_KEYS, first=22, sections=_FREMLP_SECTIONS, tail=("workspace", "saved_bytes", "saved_hidden_offset"))


def _fremlp_shape(B: int, nc: int, expand: int, H: int, W: int, dtype_code: int) -> L.FremlpShape:
    return L.FremlpShape(B, nc, expand, H, W, dtype_code)


def fremlp_plan(B: int, nc: int, expand: int, H: int, W: int, dtype: torch.dtype = torch.float32) -> dict:
    """What fremlp_fwd / fremlp_bwd launch for x [B, nc, H, W] (mi_fremlp_plan: the plan the launchers follow; no GPU work).
    ``sections`` maps each workspace section to its (byte offset, bytes)."""
    return _plan_report(L.lib().mi_fremlp_plan, _fremlp_shape(B, nc, expand, H, W, _dtype_code(dtype)), "fremlp_plan", **_FREMLP_PLAN)


def fremlp_sizes(B: int, nc: int, expand: int, H: int, W: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one FreMLP; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = _fremlp_shape(B, nc, expand, H, W, _dtype_code(dtype))
    return _sizes(L.lib().mi_fremlp_saved_bytes, L.lib().mi_fremlp_workspace, s)


def _fremlp_args(x: Tensor, params: Sequence[Tensor]):
    w1, b1, w2, b2 = params
    if x.dim() != 4:
        raise ValueError(f"fremlp: x must be [B, nc, H, W], got {tuple(x.shape)}")
    B, nc, H, W = x.shape
    hc = w1.shape[0]
    if hc % nc or tuple(w1.shape[:2]) != (hc, nc) or tuple(w2.shape[:2]) != (nc, hc) or b1.numel() != hc or b2.numel() != nc:
        raise ValueError(f"fremlp: parameters {tuple(w1.shape)}, {tuple(b1.shape)}, {tuple(w2.shape)}, {tuple(b2.shape)} do not "
                         f"fit nc = {nc}")
    s = _fremlp_shape(B, nc, hc // nc, H, W, _dt(x))
    return s, _covered(L.lib().mi_fremlp_workspace, s)


def fremlp_fwd(x: Tensor, params: Sequence[Tensor], need_saved: bool):
    """DarkIR FreMLP.forward: irfft2(MLP(|rfft2 x|) * rfft2 x / |rfft2 x|).  params: W1 [e nc, nc(, 1, 1)], b1, W2 [nc, e nc(, 1, 1)],
    b2 (fp32).  -> (out, saved)."""
    _gpu(x, *params)
    for t in params:
        _f32(t, "FreMLP parameter")
    s, ws_bytes = _fremlp_args(x, params)
    lib = L.lib()
    out, saved, ws = _out_saved_ws(x, s, lib.mi_fremlp_saved_bytes, need_saved, ws_bytes)
    w1, b1, w2, b2 = params
    L.check(lib.mi_fremlp_fwd(C.byref(s), _p(w1), _p(b1), _p(w2), _p(b2), _p(x), _p(out), _p(saved), _p(ws), _stream()), "fremlp_fwd")
    return out, saved


def fremlp_bwd(dout: Tensor, params: Sequence[Tensor], saved: Tensor, grads: Sequence[Tensor], accumulate: bool) -> Tensor:
    """Backward of fremlp_fwd: dx; the four parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(dout, saved, *params, *grads)
    for t in (*params, *grads):
        _f32(t, "FreMLP parameter / gradient")
    s, ws_bytes = _fremlp_args(dout, params)
    lib = L.lib()
    dx, ws = _out_ws(dout, ws_bytes)
    w1, _, w2, b2 = params
    L.check(lib.mi_fremlp_bwd(C.byref(s), _p(w1), _p(w2), _p(b2), _p(dout), _p(dx), *[_p(g) for g in grads], int(accumulate),
                              _p(saved), _p(ws), _stream()), "fremlp_bwd")
    return dx


# ----------------------------------------------------------------------------- SFHformer: FourierUnit
FOURIER_UNIT_MAX_C, FOURIER_UNIT_MAX_GROUPS = 256, 8
_FU_PLAN_KEYS = ("planes", "K", "channels", "groups", "group_width", "elements", "bins", "block", "bn_chunk", "chunks_per_plane",
                 "partials_per_channel", "grid_elements", "grid_bins", "kernels_fwd", "kernels_bwd", "lib_calls_fwd", "lib_calls_bwd")
_FU_SECTIONS = ("dft_tables", "dft_T", "Z", "U", "t", "ts", "pre", "q", "s", "dlogit", "stat", "bn_partials", "w_fold", "grad_tmp", "bwd_partials",
                "pw_ws", "gram_ws", "chan_sum_ws")
_FU_PLAN = dict(keys=_FU_PLAN_KEYS, first=18, sections=_FU_SECTIONS, tail=("workspace", "saved_bytes", "saved_stat_offset"))


def _fu_shape(B: int, c: int, groups: int, H: int, W: int, dtype_code: int, training: bool = True, eps: float = 1e-5,
              momentum: float = 0.1) -> L.FourierUnitShape:
    return L.FourierUnitShape(B, c, groups, H, W, dtype_code, int(training), eps, momentum)


def fourier_unit_plan(B: int, c: int, groups: int, H: int, W: int, dtype: torch.dtype = torch.float32) -> dict:
    """What fourier_unit_fwd / fourier_unit_bwd launch for x [B, c, H, W] (mi_fourier_unit_plan; no GPU work).  ``sections`` maps
    each workspace section to its (byte offset, bytes)."""
    return _plan_report(L.lib().mi_fourier_unit_plan, _fu_shape(B, c, groups, H, W, _dtype_code(dtype)), "fourier_unit_plan", **_FU_PLAN)


def fourier_unit_sizes(B: int, c: int, groups: int, H: int, W: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one FourierUnit; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = _fu_shape(B, c, groups, H, W, _dtype_code(dtype))
    return _sizes(L.lib().mi_fourier_unit_saved_bytes, L.lib().mi_fourier_unit_workspace, s)


def _fu_args(x: Tensor, params: Sequence[Tensor], training: bool, eps: float, momentum: float):
    """params: bn.weight, bn.bias, fdc.weight, fdc.bias, the gate conv's weight and bias, fpe.weight, fpe.bias."""
    bn_w, bn_b, fdc_w, fdc_b, gate_w, gate_b, fpe_w, fpe_b = params
    if x.dim() != 4:
        raise ValueError(f"fourier_unit: x must be [B, c, H, W], got {tuple(x.shape)}")
    B, c, H, W = x.shape
    G, C2 = gate_w.shape[0], 2 * c
    if G < 1 or C2 % G or (bn_w.numel(), bn_b.numel(), fdc_b.numel(), gate_b.numel(), fpe_b.numel()) != (C2, C2, G * C2, G, C2) or \
            tuple(fdc_w.shape[:2]) != (G * C2, C2 // G) or gate_w.numel() != G * C2 or fpe_w.numel() != 9 * C2:
        raise ValueError(f"fourier_unit: parameters {[tuple(p.shape) for p in params]} do not fit c = {c}")
    s = _fu_shape(B, c, G, H, W, _dt(x), training, eps, momentum)
    return s, _covered(L.lib().mi_fourier_unit_workspace, s)


def fourier_unit_fwd(x: Tensor, params: Sequence[Tensor], running_mean: Tensor, running_var: Tensor, training: bool,
                     need_saved: bool, eps: float = 1e-5, momentum: float = 0.1):
    """SFHformer FourierUnit.forward (see mi_restore.h).  ``running_mean`` / ``running_var`` [2c] fp32 are updated in place when
    ``training``.  -> (out, saved)."""
    _gpu(x, running_mean, running_var, *params)
    for t in (*params, running_mean, running_var):
        _f32(t, "FourierUnit parameter / running statistic")
    s, ws_bytes = _fu_args(x, params, training, eps, momentum)
    if running_mean.numel() != 2 * x.shape[1] or running_var.numel() != 2 * x.shape[1]:
        raise ValueError("fourier_unit: the running statistics must hold 2c values")
    lib = L.lib()
    out, saved, ws = _out_saved_ws(x, s, lib.mi_fourier_unit_saved_bytes, need_saved, ws_bytes)
    pp = _f32_struct(L.FourierUnitParams, params, "FourierUnit parameter")
    L.check(lib.mi_fourier_unit_fwd(C.byref(s), C.byref(pp), _p(x), _p(out), _p(running_mean), _p(running_var), _p(saved), _p(ws),
                                    _stream()), "fourier_unit_fwd")
    return out, saved


def fourier_unit_bwd(dout: Tensor, params: Sequence[Tensor], saved: Tensor, grads: Sequence[Tensor], accumulate: bool,
                     training: bool, eps: float = 1e-5, momentum: float = 0.1) -> Tensor:
    """Backward of fourier_unit_fwd: dx; the eight parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(dout, saved, *params, *grads)
    s, ws_bytes = _fu_args(dout, params, training, eps, momentum)
    lib = L.lib()
    dx, ws = _out_ws(dout, ws_bytes)
    pp = _f32_struct(L.FourierUnitParams, params, "FourierUnit parameter")
    gg = _f32_struct(L.FourierUnitGrads, grads, "FourierUnit gradient", int(accumulate))
    L.check(lib.mi_fourier_unit_bwd(C.byref(s), C.byref(pp), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()),
            "fourier_unit_bwd")
    return dx


# ----------------------------------------------------------------------------- SFHformer: FFN and TokenMixer_For_Local
SFH_FFN_MAX_DIM = 256
_SF_PLAN_KEYS = ("tile_w", "tile_h", "segments", "segment_width", "halo0", "halo1", "halo2", "halo3", "tiles_x", "tiles_y", "grid_x",
                 "grid_y", "grid_z", "splits", "partial_rows", "partial_cols", "kernels_fwd", "kernels_bwd", "lib_calls_fwd",
                 "lib_calls_bwd", "lds_fwd", "lds_bwd", "block")
_SF_SECTIONS = ("pw_ws", "gram_ws", "chan_sum_ws", "partials", "g", "dg", "dh")
_SF_PLAN = dict(keys=_SF_PLAN_KEYS, first=24, sections=_SF_SECTIONS, tail=("workspace", "saved_bytes", "saved_u_offset"))


def _sf_plan(fn, shape, who: str) -> dict:
    """The report with the four halo scalars folded into one ``halo`` tuple, one entry per segment, after the other scalars."""
    plan = _plan_report(fn, shape, who, **_SF_PLAN)
    halo = tuple(plan.pop(f"halo{k}") for k in range(4))[:plan["segments"]]
    items = list(plan.items())
    at = list(plan).index("sections")
    return dict(items[:at] + [("halo", halo)] + items[at:])


def sfh_ffn_plan(B: int, dim: int, H: int, W: int, dtype: torch.dtype = torch.float32) -> dict:
    """What sfh_ffn_fwd / sfh_ffn_bwd launch for x [B, dim, H, W] (mi_sfh_ffn_plan; no GPU work): the tile, the halo per segment,
    grids, backward splits, partial rows, launch counts; ``sections`` maps each workspace section to its (byte offset, bytes)."""
    return _sf_plan(L.lib().mi_sfh_ffn_plan, L.SfhFfnShape(B, dim, H, W, _dtype_code(dtype)), "sfh_ffn_plan")


def sfh_local_plan(B: int, dim: int, H: int, W: int, dtype: torch.dtype = torch.float32) -> dict:
    """The same for sfh_local_fwd / sfh_local_bwd (mi_sfh_local_plan); its workspace holds the partial rows only."""
    return _sf_plan(L.lib().mi_sfh_local_plan, L.SfhLocalShape(B, dim, H, W, _dtype_code(dtype)), "sfh_local_plan")


def sfh_ffn_sizes(B: int, dim: int, H: int, W: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one SFHformer FFN; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = L.SfhFfnShape(B, dim, H, W, _dtype_code(dtype))
    return _sizes(L.lib().mi_sfh_ffn_saved_bytes, L.lib().mi_sfh_ffn_workspace, s)


def _sf_args(x: Tensor, params: Sequence[Tensor], local: bool):
    if x.dim() != 4:
        raise ValueError(f"sfh: x must be [B, dim, H, W], got {tuple(x.shape)}")
    B, dim, H, W = x.shape
    s = dim // 2
    if local:
        want = [(s, 1, 3, 3), (s,), (s, 1, 3, 3), (s,)]
    else:
        want = [(2 * dim, dim, 1, 1), (2 * dim,), (s, 1, 3, 3), (s,), (s, 1, 5, 5), (s,), (s, 1, 7, 7), (s,), (dim, 2 * dim, 1, 1), (dim,)]
    if dim % 2 == 0 and [tuple(p.shape) for p in params] != want:
        raise ValueError(f"sfh: parameters {[tuple(p.shape) for p in params]} do not fit dim = {dim}")
    lib = L.lib()
    shape = (L.SfhLocalShape if local else L.SfhFfnShape)(B, dim, H, W, _dt(x))
    return shape, _covered(lib.mi_sfh_local_workspace if local else lib.mi_sfh_ffn_workspace, shape)


def sfh_ffn_fwd(x: Tensor, params: Sequence[Tensor], need_saved: bool):
    """SFHformer FFN.forward (see mi_restore.h).  params: conv_init, conv1_1, conv1_2, conv1_3, conv_fina weights and biases.
    -> (out, saved): the blob holds h and u in x's dtype."""
    _gpu(x, *params)
    s, ws_bytes = _sf_args(x, params, False)
    lib = L.lib()
    out, saved, ws = _out_saved_ws(x, s, lib.mi_sfh_ffn_saved_bytes, need_saved, ws_bytes)
    pp = _f32_struct(L.SfhFfnParams, params, "SFHformer FFN parameter")
    L.check(lib.mi_sfh_ffn_fwd(C.byref(s), C.byref(pp), _p(x), _p(out), _p(saved), _p(ws), _stream()), "sfh_ffn_fwd")
    return out, saved


def sfh_ffn_bwd(x: Tensor, dout: Tensor, params: Sequence[Tensor], saved: Tensor, grads: Sequence[Tensor], accumulate: bool) -> Tensor:
    """Backward of sfh_ffn_fwd: dx; the ten parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(x, dout, saved, *params, *grads)
    s, ws_bytes = _sf_args(x, params, False)
    lib = L.lib()
    dx, ws = _out_ws(x, ws_bytes)
    pp = _f32_struct(L.SfhFfnParams, params, "SFHformer FFN parameter")
    gg = _f32_struct(L.SfhFfnGrads, grads, "SFHformer FFN gradient", int(accumulate))
    L.check(lib.mi_sfh_ffn_bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()),
            "sfh_ffn_bwd")
    return dx


def sfh_local_fwd(x: Tensor, params: Sequence[Tensor]) -> Tensor:
    """SFHformer TokenMixer_For_Local.forward.  params: CDilated_1 and CDilated_2 weights and biases.  Saves nothing but x."""
    _gpu(x, *params)
    s, ws_bytes = _sf_args(x, params, True)
    out, ws = _out_ws(x, ws_bytes)
    pp = _f32_struct(L.SfhLocalParams, params, "SFHformer local mixer parameter")
    L.check(L.lib().mi_sfh_local_fwd(C.byref(s), C.byref(pp), _p(x), _p(out), _p(ws), _stream()), "sfh_local_fwd")
    return out


def sfh_local_bwd(x: Tensor, dout: Tensor, params: Sequence[Tensor], grads: Sequence[Tensor], accumulate: bool) -> Tensor:
    """Backward of sfh_local_fwd: dx; the four parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(x, dout, *params, *grads)
    s, ws_bytes = _sf_args(x, params, True)
    dx, ws = _out_ws(x, ws_bytes)
    pp = _f32_struct(L.SfhLocalParams, params, "SFHformer local mixer parameter")
    gg = _f32_struct(L.SfhLocalGrads, grads, "SFHformer local mixer gradient", int(accumulate))
    L.check(L.lib().mi_sfh_local_bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(ws), _stream()),
            "sfh_local_bwd")
    return dx


# ----------------------------------------------------------------------------- SFHformer: TokenMixer_For_Gloal and Mixer
SFH_MIXER_MAX_DIM, SFH_MIXER_MIN_HW, SFH_MIXER_MAX_HW = 128, 2, 512
_SM_PLAN_KEYS = ("mode", "B", "dim", "channels", "N", "pool", "grid_flat_dim", "grid_flat_2dim", "grid_tail_back", "block", "kernels_fwd",
                 "kernels_bwd", "lib_calls_fwd", "lib_calls_bwd", "bwd_scratch_bytes")
_SM_SECTIONS = ("pw_ws", "gram_ws", "chan_sum_ws", "fu_ws", "local_ws", "p", "f", "g", "small", "fold", "gram_out", "pool_partials",
                "scratch")
_SM_SAVED = ("a", "b", "l", "u1", "r", "u2", "fu_blob")
_SM_PLAN = dict(keys=_SM_PLAN_KEYS, first=16, sections=_SM_SECTIONS, saved=(44, _SM_SAVED))


def _sm_shape(B: int, dim: int, H: int, W: int, dtype_code: int, training: bool = True, eps: float = 1e-5,
              momentum: float = 0.1) -> L.SfhMixerShape:
    return L.SfhMixerShape(B, dim, H, W, dtype_code, int(training), eps, momentum)


def sfh_global_plan(B: int, dim: int, H: int, W: int, dtype: torch.dtype = torch.float32) -> dict:
    """What sfh_global_fwd / sfh_global_bwd launch for x [B, dim, H, W] (mi_sfh_global_plan; no GPU work): grids, launch counts,
    ``sections`` (workspace) and ``saved_sections`` (the blob), each name -> (byte offset, bytes)."""
    return _plan_report(L.lib().mi_sfh_global_plan, _sm_shape(B, dim, H, W, _dtype_code(dtype)), "sfh_global_plan", **_SM_PLAN)


def sfh_mixer_plan(B: int, dim: int, H: int, W: int, dtype: torch.dtype = torch.float32) -> dict:
    """The same for sfh_mixer_fwd / sfh_mixer_bwd (mi_sfh_mixer_plan)."""
    return _plan_report(L.lib().mi_sfh_mixer_plan, _sm_shape(B, dim, H, W, _dtype_code(dtype)), "sfh_mixer_plan", **_SM_PLAN)


def sfh_global_sizes(B: int, dim: int, H: int, W: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one TokenMixer_For_Gloal; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = _sm_shape(B, dim, H, W, _dtype_code(dtype))
    return _sizes(L.lib().mi_sfh_global_saved_bytes, L.lib().mi_sfh_global_workspace, s)


def sfh_mixer_sizes(B: int, dim: int, H: int, W: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one Mixer; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = _sm_shape(B, dim, H, W, _dtype_code(dtype))
    return _sizes(L.lib().mi_sfh_mixer_saved_bytes, L.lib().mi_sfh_mixer_workspace, s)


def _sm_global_shapes(dim: int):
    c2 = 4 * dim                                              # spectral channels of FourierUnit(2 dim, 2 dim)
    return [(2 * dim, dim, 1, 1), (2 * dim,), (dim, 2 * dim, 1, 1), (dim,), (c2,), (c2,), (4 * c2, c2 // 4, 1, 1), (4 * c2,),
            (4, c2, 1, 1), (4,), (c2, 1, 3, 3), (c2,)]


def _sm_args(x: Tensor, params: Sequence[Tensor], mixer: bool, training: bool, eps: float, momentum: float):
    if x.dim() != 4:
        raise ValueError(f"sfh: x must be [B, dim, H, W], got {tuple(x.shape)}")
    B, dim, H, W = x.shape
    want = _sm_global_shapes(dim)
    if mixer:
        s = dim // 2
        want = [(s, 1, 3, 3), (s,), (s, 1, 3, 3), (s,)] + want + [(dim, 2 * dim, 1, 1), (dim,), (dim, 2 * dim, 1, 1), (dim,),
                                                                 (2 * dim, dim, 1, 1), (2 * dim,), (2 * dim, dim, 1, 1), (2 * dim,)]
    # (an odd Mixer dim has no parameter list of its own: the channel count is still held against conv_init's, so that a wrong
    # count is a ValueError and only a module that IS odd reaches the library's refusal)
    fits = params[-2].dim() == 4 and params[-2].shape[1] == dim if mixer and dim % 2 else [tuple(p.shape) for p in params] == want
    if not fits:
        raise ValueError(f"sfh: parameters {[tuple(p.shape) for p in params]} do not fit dim = {dim}")
    lib = L.lib()
    shape = _sm_shape(B, dim, H, W, _dt(x), training, eps, momentum)
    return shape, _covered(lib.mi_sfh_mixer_workspace if mixer else lib.mi_sfh_global_workspace, shape)


def _sm_fwd(mixer: bool, x, params, running_mean, running_var, training, need_saved, eps, momentum):
    _gpu(x, running_mean, running_var, *params)
    _f32(running_mean, "FourierUnit running statistic"), _f32(running_var, "FourierUnit running statistic")
    s, ws_bytes = _sm_args(x, params, mixer, training, eps, momentum)
    if running_mean.numel() != 4 * x.shape[1] or running_var.numel() != 4 * x.shape[1]:
        raise ValueError("sfh: the running statistics must hold 4 dim values")
    lib = L.lib()
    sized, fwd, cls, who = ((lib.mi_sfh_mixer_saved_bytes, lib.mi_sfh_mixer_fwd, L.SfhMixerParams, "sfh_mixer_fwd") if mixer else
                            (lib.mi_sfh_global_saved_bytes, lib.mi_sfh_global_fwd, L.SfhGlobalParams, "sfh_global_fwd"))
    out, saved, ws = _out_saved_ws(x, s, sized, need_saved, ws_bytes)
    pp = _f32_struct(cls, params, "SFHformer mixer parameter")
    L.check(fwd(C.byref(s), C.byref(pp), _p(x), _p(out), _p(running_mean), _p(running_var), _p(saved), _p(ws), _stream()), who)
    return out, saved


def _sm_bwd(mixer: bool, x, dout, params, saved, grads, accumulate, training, eps, momentum):
    _gpu(x, dout, saved, *params, *grads)
    s, ws_bytes = _sm_args(x, params, mixer, training, eps, momentum)
    lib = L.lib()
    dx, ws = _out_ws(x, ws_bytes)
    bwd, pcls, gcls, who = ((lib.mi_sfh_mixer_bwd, L.SfhMixerParams, L.SfhMixerGrads, "sfh_mixer_bwd") if mixer else
                            (lib.mi_sfh_global_bwd, L.SfhGlobalParams, L.SfhGlobalGrads, "sfh_global_bwd"))
    pp = _f32_struct(pcls, params, "SFHformer mixer parameter")
    gg = _f32_struct(gcls, grads, "SFHformer mixer gradient", int(accumulate))
    L.check(bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()), who)
    return dx


def sfh_global_fwd(x: Tensor, params: Sequence[Tensor], running_mean: Tensor, running_var: Tensor, training: bool, need_saved: bool,
                   eps: float = 1e-5, momentum: float = 0.1):
    """SFHformer TokenMixer_For_Gloal.forward (see mi_restore.h).  params: conv_init, conv_fina, then the FourierUnit's eight (the
    module's named_parameters() order); ``running_mean`` / ``running_var`` [4 dim] fp32 are updated in place when ``training``.
    -> (out, saved)."""
    return _sm_fwd(False, x, params, running_mean, running_var, training, need_saved, eps, momentum)


def sfh_global_bwd(x: Tensor, dout: Tensor, params: Sequence[Tensor], saved: Tensor, grads: Sequence[Tensor], accumulate: bool,
                   training: bool, eps: float = 1e-5, momentum: float = 0.1) -> Tensor:
    """Backward of sfh_global_fwd: dx; the twelve parameter gradients are written (accumulate: added) into ``grads``."""
    return _sm_bwd(False, x, dout, params, saved, grads, accumulate, training, eps, momentum)


def sfh_mixer_fwd(x: Tensor, params: Sequence[Tensor], running_mean: Tensor, running_var: Tensor, training: bool, need_saved: bool,
                  eps: float = 1e-5, momentum: float = 0.1):
    """SFHformer Mixer.forward (see mi_restore.h).  params: the 24 of the module's named_parameters() order (mixer_local,
    mixer_gloal, ca_conv, ca.1, ca.3, conv_init); the running statistics are those of mixer_gloal.FFC.bn.  -> (out, saved)."""
    return _sm_fwd(True, x, params, running_mean, running_var, training, need_saved, eps, momentum)


def sfh_mixer_bwd(x: Tensor, dout: Tensor, params: Sequence[Tensor], saved: Tensor, grads: Sequence[Tensor], accumulate: bool,
                  training: bool, eps: float = 1e-5, momentum: float = 0.1) -> Tensor:
    """Backward of sfh_mixer_fwd: dx; the 24 parameter gradients are written (accumulate: added) into ``grads``."""
    return _sm_bwd(True, x, dout, params, saved, grads, accumulate, training, eps, momentum)


# ----------------------------------------------------------------------------- SFHformer: the Block's BatchNorm2d and scaled residual
BN2D_MAX_C = 4096
_BN_PLAN_KEYS = ("B", "C", "N", "dtype", "training", "block", "chunk", "chunks_per_plane", "partials_per_channel", "vector_width",
                 "chunks", "grid_chunks", "grid_channels", "launches_fwd", "launches_fwd_part_in", "launches_bwd")
_BN_SECTIONS = ("partials", "stat", "bwd_means")
_BN_PLAN = dict(keys=_BN_PLAN_KEYS, first=16, sections=_BN_SECTIONS, tail=("workspace", "stat_bytes", "pair_bytes"))


def _bn_shape(B: int, Cn: int, H: int, W: int, dtype_code: int, training: bool = True, eps: float = 1e-5,
              momentum: float = 0.1) -> L.Bn2dShape:
    return L.Bn2dShape(B, Cn, H, W, dtype_code, int(training), eps, momentum)


def bn2d_plan(B: int, Cn: int, H: int, W: int, dtype: torch.dtype = torch.float32, training: bool = True) -> dict:
    """What bn2d_fwd / bn2d_bwd launch for x [B, C, H, W] (mi_bn2d_plan; no GPU work): the chunk size, chunks per plane, partials per
    channel, the vector width the shape allows, grids, launch counts; ``sections`` maps each workspace section to its (byte offset,
    bytes); ``pair_bytes``: what ``part_in`` / ``part_out`` hold."""
    return _plan_report(L.lib().mi_bn2d_plan, _bn_shape(B, Cn, H, W, _dtype_code(dtype), training), "bn2d_plan", **_BN_PLAN)


def scale_res_plan(B: int, Cn: int, H: int, W: int, dtype: torch.dtype = torch.float32) -> dict:
    """The same for scale_res_fwd / scale_res_bwd (mi_scale_res_plan); its workspace holds the backward's partial sums only."""
    return _plan_report(L.lib().mi_scale_res_plan, _bn_shape(B, Cn, H, W, _dtype_code(dtype)), "scale_res_plan", **_BN_PLAN)


def bn2d_workspace(B: int, Cn: int, H: int, W: int, dtype: torch.dtype, training: bool = True) -> int:
    """Workspace bytes of one BatchNorm2d call; 0 for a shape the kernels refuse.  No GPU needed."""
    s = _bn_shape(B, Cn, H, W, _dtype_code(dtype), training)
    return int(L.lib().mi_bn2d_workspace(C.byref(s)))


def scale_res_workspace(B: int, Cn: int, H: int, W: int, dtype: torch.dtype) -> int:
    s = _bn_shape(B, Cn, H, W, _dtype_code(dtype))
    return int(L.lib().mi_scale_res_workspace(C.byref(s)))


def _bn_args(who: str, x: Tensor, per_channel: Sequence[Optional[Tensor]], sizer, training: bool, eps: float, momentum: float):
    """The shape struct and workspace bytes for x [B, C, H, W]; ``per_channel``: fp32 tensors that must hold C values."""
    if x.dim() != 4:
        raise ValueError(f"{who}: x must be [B, C, H, W], got {tuple(x.shape)}")
    B, Cn, H, W = x.shape
    for t in per_channel:
        if t is not None and _f32(t, f"{who} parameter / statistic").numel() != Cn:
            raise ValueError(f"{who}: a per-channel tensor of shape {tuple(t.shape)} does not fit C = {Cn}")
    s = _bn_shape(B, Cn, H, W, _dt(x), training, eps, momentum)
    return s, _covered(sizer, s)


def _same(who: str, x: Tensor, *others: Optional[Tensor]) -> None:
    for t in others:
        if t is not None and (t.shape != x.shape or t.dtype != x.dtype):
            raise ValueError(f"{who}: tensors differ in shape or dtype ({tuple(t.shape)} {t.dtype} against {tuple(x.shape)} {x.dtype})")


def bn2d_fwd(x: Tensor, weight: Tensor, bias: Tensor, running_mean: Tensor, running_var: Tensor, training: bool, need_stat: bool,
             eps: float = 1e-5, momentum: float = 0.1, part_in: Optional[Tensor] = None):
    """BatchNorm2d.forward over x [B, C, H, W] (see mi_restore.h).  ``running_mean`` / ``running_var`` [C] fp32 are updated in place
    when ``training``.  ``part_in``: the (mean, M2) pairs of x as ``scale_res_fwd(..., want_part=True)`` returns them; the statistics
    pass is skipped.  -> (y, stat); stat [2C] = (mu, r) is what bn2d_bwd needs beside x (None unless ``need_stat``)."""
    _gpu(x, weight, bias, running_mean, running_var, part_in)
    lib = L.lib()
    s, ws_bytes = _bn_args("bn2d", x, (weight, bias, running_mean, running_var), lib.mi_bn2d_workspace, training, eps, momentum)
    if part_in is not None and (part_in.dtype != torch.float32 or part_in.numel() * 4 != bn2d_plan(*x.shape, x.dtype, training)["pair_bytes"]):
        raise ValueError("bn2d: part_in must hold the plan's fp32 (mean, M2) pairs")
    y = torch.empty_like(x)
    stat = torch.empty(2 * x.shape[1], dtype=torch.float32, device=x.device) if need_stat else None
    ws = _ws(ws_bytes, x.device)
    L.check(lib.mi_bn2d_fwd(C.byref(s), _p(weight), _p(bias), _p(x), _p(y), _p(running_mean), _p(running_var), _p(stat), _p(part_in),
                            _p(ws), _stream()), "bn2d_fwd")
    return y, stat


def bn2d_bwd(x: Tensor, dy: Tensor, weight: Tensor, stat: Tensor, grads: Sequence[Tensor], accumulate: bool, training: bool,
             eps: float = 1e-5, momentum: float = 0.1, dres: Optional[Tensor] = None) -> Tensor:
    """Backward of bn2d_fwd: dx (``dres`` given: dx + dres, added in fp32 and rounded once); dw and db are written (accumulate: added)
    into ``grads``."""
    dw, db = grads
    _gpu(x, dy, weight, stat, dw, db, dres)
    _same("bn2d", x, dy, dres)
    lib = L.lib()
    s, ws_bytes = _bn_args("bn2d", x, (weight, dw, db), lib.mi_bn2d_workspace, training, eps, momentum)
    if _f32(stat, "bn2d stat").numel() != 2 * x.shape[1]:
        raise ValueError("bn2d: stat must hold 2C values")
    dx, ws = _out_ws(x, ws_bytes)
    L.check(lib.mi_bn2d_bwd(C.byref(s), _p(weight), _p(x), _p(dy), _p(dres), _p(dx), _p(dw), _p(db), int(accumulate), _p(stat), _p(ws),
                            _stream()), "bn2d_bwd")
    return dx


def scale_res_fwd(f: Tensor, x: Tensor, scale: Tensor, want_part: bool = False):
    """out = f scale[c] + x (``scale``: C fp32 values).  ``want_part``: -> (out, part), part the BatchNorm (mean, M2) pairs of out as
    stored, for ``bn2d_fwd(..., part_in=part)``; else -> out."""
    _gpu(f, x, scale)
    _same("scale_res", f, x)
    lib = L.lib()
    s, _ = _bn_args("scale_res", f, (scale,), lib.mi_scale_res_workspace, True, 1e-5, 0.1)
    out = torch.empty_like(f)
    part = torch.empty(bn2d_plan(*f.shape, f.dtype, False)["pair_bytes"] // 4, dtype=torch.float32, device=f.device) if want_part else None
    L.check(lib.mi_scale_res_fwd(C.byref(s), _p(scale), _p(f), _p(x), _p(out), _p(part), _stream()), "scale_res_fwd")
    return (out, part) if want_part else out


def scale_res_bwd(f: Tensor, dout: Tensor, scale: Tensor, dscale: Tensor, accumulate: bool) -> Tensor:
    """Backward of scale_res_fwd: df = dout scale[c]; sum f dout is written (accumulate: added) into ``dscale``.  The gradient towards
    x is ``dout`` itself."""
    _gpu(f, dout, scale, dscale)
    _same("scale_res", f, dout)
    lib = L.lib()
    s, ws_bytes = _bn_args("scale_res", f, (scale, dscale), lib.mi_scale_res_workspace, True, 1e-5, 0.1)
    df = torch.empty_like(f)
    ws = _ws(ws_bytes, f.device)
    L.check(lib.mi_scale_res_bwd(C.byref(s), _p(scale), _p(f), _p(dout), _p(df), _p(dscale), int(accumulate), _p(ws), _stream()),
            "scale_res_bwd")
    return df


# ----------------------------------------------------------------------------- SFHformer: Block
SFH_BLOCK_MAX_DIM, SFH_BLOCK_MIN_HW, SFH_BLOCK_MAX_HW = SFH_MIXER_MAX_DIM, SFH_MIXER_MIN_HW, SFH_MIXER_MAX_HW
SFH_BLOCK_PARAMS = 40                                         # beta, gamma, norm1, norm2 (weight, bias), the Mixer's 24, the FFN's 10
_SB_PLAN_KEYS = ("B", "dim", "N", "chunks_per_plane", "lib_calls_fwd", "lib_calls_fwd_part_in", "lib_calls_bwd", "kernels_fwd",
                 "kernels_fwd_part_in", "kernels_bwd", "sub_lib_calls_fwd", "sub_lib_calls_bwd")
_SB_SECTIONS = ("sub_ws", "p1", "d0", "d1", "d2", "scratch")
_SB_SAVED = ("y1", "m", "x1", "y2", "f", "stat1", "stat2", "mixer_blob", "ffn_blob")
_SB_PLAN = dict(keys=_SB_PLAN_KEYS, first=16, sections=_SB_SECTIONS, saved=(32, _SB_SAVED), tail=("workspace", "saved_bytes", "pair_bytes"))


def sfh_block_plan(B: int, dim: int, H: int, W: int, dtype: torch.dtype = torch.float32, training: bool = True) -> dict:
    """What sfh_block_fwd / sfh_block_bwd run for x [B, dim, H, W] (mi_sfh_block_plan; no GPU work): library calls, the kernel launches
    summed from the parts' plans, ``sections`` (workspace) and ``saved_sections`` (the blob), each name -> (byte offset, bytes);
    ``pair_bytes``: what ``part_in`` / ``part_out`` hold."""
    return _plan_report(L.lib().mi_sfh_block_plan, _sm_shape(B, dim, H, W, _dtype_code(dtype), training), "sfh_block_plan", **_SB_PLAN)


def sfh_block_sizes(B: int, dim: int, H: int, W: int, dtype: torch.dtype, training: bool = True) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one Block; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = _sm_shape(B, dim, H, W, _dtype_code(dtype), training)
    return _sizes(L.lib().mi_sfh_block_saved_bytes, L.lib().mi_sfh_block_workspace, s)


@functools.lru_cache(maxsize=None)
def _sb_pairs(B: int, dim: int, H: int, W: int, dtype: torch.dtype) -> int:
    """fp32 values in the pair buffer of x [B, dim, H, W] (a property of the shape: asked once)."""
    return sfh_block_plan(B, dim, H, W, dtype, True)["pair_bytes"] // 4


def _sb_struct(cls, ts: Sequence[Tensor], what: str, *tail):
    """mi_sfh_block_params / _grads from the 40 tensors in the Block's named_parameters() order."""
    beta, gamma, n1w, n1b, n2w, n2b = ts[:6]
    mixer, ffn = ts[6:30], ts[30:40]
    grads = cls is L.SfhBlockGrads
    mx = _f32_struct(L.SfhMixerGrads if grads else L.SfhMixerParams, mixer, what, *tail)
    ff = _f32_struct(L.SfhFfnGrads if grads else L.SfhFfnParams, ffn, what, *tail)
    for t in ts[:6]:
        _f32(t, what)
    return cls(_p(n1w), _p(n1b), mx, _p(beta), _p(n2w), _p(n2b), ff, _p(gamma), *tail)


def _sb_args(x: Tensor, params: Sequence[Tensor], training: bool, eps: float, momentum: float):
    if x.dim() != 4:
        raise ValueError(f"sfh_block: x must be [B, dim, H, W], got {tuple(x.shape)}")
    B, dim, H, W = x.shape
    s = dim // 2
    want = ([(1, dim, 1, 1)] * 2 + [(dim,)] * 4 + [(s, 1, 3, 3), (s,), (s, 1, 3, 3), (s,)] + _sm_global_shapes(dim) +
            [(dim, 2 * dim, 1, 1), (dim,), (dim, 2 * dim, 1, 1), (dim,), (2 * dim, dim, 1, 1), (2 * dim,), (2 * dim, dim, 1, 1), (2 * dim,)] +
            [(2 * dim, dim, 1, 1), (2 * dim,), (s, 1, 3, 3), (s,), (s, 1, 5, 5), (s,), (s, 1, 7, 7), (s,), (dim, 2 * dim, 1, 1), (dim,)])
    if len(params) != SFH_BLOCK_PARAMS or (dim % 2 == 0 and [tuple(p.shape) for p in params] != want):
        raise ValueError(f"sfh_block: parameters {[tuple(p.shape) for p in params]} do not fit dim = {dim}")
    shape = _sm_shape(B, dim, H, W, _dt(x), training, eps, momentum)
    return shape, _covered(L.lib().mi_sfh_block_workspace, shape)


def sfh_block_fwd(x: Tensor, params: Sequence[Tensor], stats: Sequence[Tensor], training: bool, need_saved: bool, eps: float = 1e-5,
                  momentum: float = 0.1, part_in: Optional[Tensor] = None, want_part: bool = False):
    """SFHformer Block.forward (see mi_restore.h).  params: the 40 of the module's named_parameters() order (beta, gamma, norm1,
    norm2, mixer, ffn); ``stats``: running mean and var of norm1, of norm2 [dim] and of mixer.mixer_gloal.FFC.bn [4 dim], fp32,
    updated in place when ``training``.  ``part_in``: the (mean, M2) pairs of x from a producer; ``want_part``: also return those of
    out (training mode only: eval mode uses neither).  -> (out, saved, part_out)."""
    _gpu(x, part_in, *params, *stats)
    s, ws_bytes = _sb_args(x, params, training, eps, momentum)
    dim = x.shape[1]
    if len(stats) != 6 or [_f32(t, "sfh_block running statistic").numel() for t in stats] != [dim] * 4 + [4 * dim] * 2:
        raise ValueError("sfh_block: the running statistics must hold dim, dim, dim, dim, 4 dim, 4 dim values")
    lib = L.lib()
    pairs = _sb_pairs(*x.shape, x.dtype) if training and (want_part or part_in is not None) else 0
    if part_in is not None and training and (part_in.dtype != torch.float32 or part_in.numel() != pairs):
        raise ValueError("sfh_block: part_in must hold the plan's fp32 (mean, M2) pairs")
    out, saved, ws = _out_saved_ws(x, s, lib.mi_sfh_block_saved_bytes, need_saved, ws_bytes)
    part_out = torch.empty(pairs, dtype=torch.float32, device=x.device) if training and want_part else None
    pp = _sb_struct(L.SfhBlockParams, params, "SFHformer Block parameter")
    st = L.SfhBlockStats(*[_p(t) for t in stats])
    L.check(lib.mi_sfh_block_fwd(C.byref(s), C.byref(pp), _p(x), _p(out), C.byref(st), _p(part_in) if training else None, _p(part_out),
                                 _p(saved), _p(ws), _stream()), "sfh_block_fwd")
    return out, saved, part_out


def sfh_block_bwd(x: Tensor, dout: Tensor, params: Sequence[Tensor], saved: Tensor, grads: Sequence[Tensor], accumulate: bool,
                  training: bool, eps: float = 1e-5, momentum: float = 0.1) -> Tensor:
    """Backward of sfh_block_fwd: dx; the 40 parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(x, dout, saved, *params, *grads)
    _same("sfh_block", x, dout)
    s, ws_bytes = _sb_args(x, params, training, eps, momentum)
    if len(grads) != SFH_BLOCK_PARAMS:
        raise ValueError("sfh_block: 40 gradient buffers expected")
    dx, ws = _out_ws(x, ws_bytes)
    pp = _sb_struct(L.SfhBlockParams, params, "SFHformer Block parameter")
    gg = _sb_struct(L.SfhBlockGrads, grads, "SFHformer Block gradient", int(accumulate))
    L.check(L.lib().mi_sfh_block_bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()),
            "sfh_block_bwd")
    return dx


# ----------------------------------------------------------------------------- DarkIR: EBlock and its tail
EBLOCK_MAX_C, EBLOCK_MIN_HW, EBLOCK_MAX_HW = 256, 2, FREMLP_MAX_HW
_EBLOCK_PLAN_KEYS = ("x0_bytes", "xe_bytes", "x1_bytes", "g_bytes", "y_bytes", "f_bytes", "stats_bytes", "small_bytes",
                     "fremlp_blob_bytes", "saved_bytes", "workspace", "calls_fwd", "calls_bwd", "fregate_bwd_slices")


def _fregate_check(y: Tensor, *others: Tensor):
    if y.dim() != 4:
        raise ValueError(f"fregate: y must be [B, C, H, W], got {tuple(y.shape)}")
    for t in others:
        if t.shape != y.shape or t.dtype != y.dtype:
            raise ValueError(f"fregate: tensors differ in shape or dtype ({tuple(t.shape)} {t.dtype} against {tuple(y.shape)} {y.dtype})")
    B, Cc, H, W = y.shape
    return B, Cc, H * W


def fregate_fwd(y: Tensor, f: Tensor, gamma: Tensor) -> Tensor:
    """EBlock's tail: out = y * (1 + gamma[c] * f).  y, f [B, C, H, W]; gamma fp32 with C elements."""
    _gpu(y, f, gamma)
    _f32(gamma, "fregate gamma")
    B, Cc, N = _fregate_check(y, f)
    if gamma.numel() != Cc:
        raise ValueError(f"fregate: gamma has {gamma.numel()} elements for {Cc} channels")
    out = torch.empty_like(y)
    L.check(L.lib().mi_fregate_fwd(_p(y), _p(f), _p(gamma), _p(out), B, Cc, N, _dt(y), _stream()), "fregate_fwd")
    return out


def fregate_bwd(dout: Tensor, y: Tensor, f: Tensor, gamma: Tensor, dgamma: Tensor, accumulate: bool):
    """Backward of fregate_fwd in one pass -> (df, dyr): df = dout gamma y (FreMLP's cotangent), dyr = dout (1 + gamma f) (the
    residual's share); dgamma (fp32, C elements) is written (accumulate: added to) with sum_{b,p} dout y f."""
    _gpu(dout, y, f, gamma, dgamma)
    _f32(gamma, "fregate gamma"); _f32(dgamma, "fregate gradient")
    B, Cc, N = _fregate_check(y, f, dout)
    if gamma.numel() != Cc or dgamma.numel() != Cc:
        raise ValueError(f"fregate: gamma / dgamma have {gamma.numel()} / {dgamma.numel()} elements for {Cc} channels")
    lib = L.lib()
    df, dyr = torch.empty_like(y), torch.empty_like(y)
    ws = _ws(lib.mi_fregate_bwd_workspace(B, Cc, N), y.device)
    L.check(lib.mi_fregate_bwd(_p(dout), _p(y), _p(f), _p(gamma), _p(df), _p(dyr), _p(dgamma), B, Cc, N, int(accumulate), _dt(y), _p(ws),
                               _stream()), "fregate_bwd")
    return df, dyr


_eblock_shape = functools.partial(_block_shape, L.EblockShape)


def eblock_sizes(B: int, Cc: int, H: int, W: int, dtype: torch.dtype, dilations: Sequence[int], extra: bool) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one EBlock; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = _eblock_shape(B, Cc, H, W, _dtype_code(dtype), dilations, extra)
    return _sizes(L.lib().mi_eblock_saved_bytes, L.lib().mi_eblock_workspace, s)


def eblock_plan(B: int, Cc: int, H: int, W: int, dtype: torch.dtype, dilations: Sequence[int], extra: bool) -> dict:
    """Section sizes of the saved blob, the two totals and the launch counts of one EBlock (mi_eblock_plan; no GPU work)."""
    out = (L.c_i64 * 16)()
    s = _eblock_shape(B, Cc, H, W, _dtype_code(dtype), dilations, extra)
    L.check(L.lib().mi_eblock_plan(C.byref(s), out), "eblock_plan")
    return {k: int(out[i]) for i, k in enumerate(_EBLOCK_PLAN_KEYS)}


# mi_eblock_params / mi_eblock_grads from the flat list: norm1 (2), extra_conv (2, None without it), conv1 (2), the branches'
# weights (n_dil), their biases (n_dil), sca (2), conv3 (2), beta, norm2 (2), freq.process1.0 (2), freq.process1.2 (2), gamma
_eblock_struct = functools.partial(_table_struct, L.EBLOCK_FIELDS)


def _eblock_args(x: Tensor, dilations: Sequence[int], extra: bool):
    if x.dim() != 4:
        raise ValueError(f"eblock: x must be [B, c, H, W], got {tuple(x.shape)}")
    B, Cc, H, W = x.shape
    s = _eblock_shape(B, Cc, H, W, _dt(x), dilations, extra)
    return s, _covered(L.lib().mi_eblock_workspace, s)


def eblock_fwd(x: Tensor, params: Sequence[Optional[Tensor]], dilations: Sequence[int], extra: bool, need_saved: bool):
    """DarkIR EBlock.forward.  params: see _eblock_struct.  -> (out, saved)."""
    _gpu(x, *params)
    s, ws_bytes = _eblock_args(x, dilations, extra)
    lib = L.lib()
    out, saved, ws = _out_saved_ws(x, s, lib.mi_eblock_saved_bytes, need_saved, ws_bytes)
    pp = _eblock_struct(L.EblockParams, params, len(dilations), "EBlock parameter")
    L.check(lib.mi_eblock_fwd(C.byref(s), C.byref(pp), _p(x), _p(out), _p(saved), _p(ws), _stream()), "eblock_fwd")
    return out, saved


def eblock_bwd(x: Tensor, dout: Tensor, params: Sequence[Optional[Tensor]], dilations: Sequence[int], extra: bool, saved: Tensor,
               grads: Sequence[Optional[Tensor]], accumulate: bool) -> Tensor:
    """Backward of eblock_fwd: dx; the parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(x, dout, saved, *params, *grads)
    s, ws_bytes = _eblock_args(x, dilations, extra)
    lib = L.lib()
    dx, ws = _out_ws(x, ws_bytes)
    pp = _eblock_struct(L.EblockParams, params, len(dilations), "EBlock parameter")
    gg = _eblock_struct(L.EblockGrads, grads, len(dilations), "EBlock gradient", int(accumulate))
    L.check(lib.mi_eblock_bwd(C.byref(s), C.byref(pp), _p(x), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()), "eblock_bwd")
    return dx


def _dft2_ws(who: str, B: int, Cc: int, H: int, W: int, device) -> Tensor:
    n = L.lib().mi_dft2_workspace(B, Cc, H, W)
    if n == 0:
        raise NotImplementedError(f"image_restoration_amd: {who}: [{B}, {Cc}, {H}, {W}] not covered; the dense-DFT kernels take "
                                  f"2 <= H, W <= {FREMLP_MAX_HW}")
    return _ws(n, device)


def dft2_r2c(x: Tensor):
    """rfft2 of x [B, C, H, W] (fp32 or bf16) as dense-DFT GEMMs (mi_dft2_r2c) -> (Re Z, Im Z), fp32 [B, C, H, W/2 + 1]."""
    _gpu(x)
    if x.dim() != 4:
        raise ValueError(f"dft2_r2c: x must be [B, C, H, W], got {tuple(x.shape)}")
    B, Cc, H, W = x.shape
    dt = _dt(x)
    ws = _dft2_ws("dft2_r2c", B, Cc, H, W, x.device)
    zre = torch.empty(B, Cc, H, W // 2 + 1, dtype=torch.float32, device=x.device)
    zim = torch.empty_like(zre)
    L.check(L.lib().mi_dft2_r2c(_p(x), _p(zre), _p(zim), B, Cc, H, W, dt, _p(ws), _stream()), "dft2_r2c")
    return zre, zim


def dft2_c2r(yre: Tensor, yim: Tensor, W: int, dtype: torch.dtype = torch.float32) -> Tensor:
    """irfft2(yre + i yim, s=(H, W), norm='backward') of fp32 [B, C, H, W/2 + 1] halves (mi_dft2_c2r) -> [B, C, H, W] in ``dtype``."""
    _gpu(yre, yim)
    _f32(yre, "dft2_c2r input")
    _f32(yim, "dft2_c2r input")
    if yre.dim() != 4 or yre.shape != yim.shape or yre.shape[3] != W // 2 + 1:
        raise ValueError(f"dft2_c2r: the halves must be [B, C, H, {W // 2 + 1}] for W = {W}, got {tuple(yre.shape)} and "
                         f"{tuple(yim.shape)}")
    B, Cc, H, _ = yre.shape
    dt = _dtype_code(dtype)
    ws = _dft2_ws("dft2_c2r", B, Cc, H, W, yre.device)
    out = torch.empty(B, Cc, H, W, dtype=dtype, device=yre.device)
    L.check(L.lib().mi_dft2_c2r(_p(yre), _p(yim), _p(out), B, Cc, H, W, dt, _p(ws), _stream()), "dft2_c2r")
    return out


# ----------------------------------------------------------------------------- DRSformer: MEFC (one OALayer + GroupOLs pair)
MEFC_STEP_PARAMS = 23     # per OperationLayer: SepConv k = 1, 3, 5, 7 (op.0, op.1, op.3, op.4), DilConv k = 3, 5, 7 (op.0, op.1), _out.0


def _mefc_shape(x: Tensor, steps: int) -> L.MefcShape:
    B, Cc, H, W = x.shape
    return L.MefcShape(B, Cc, H, W, _dt(x), int(steps))


def _mefc_steps(ts: Sequence[Optional[Tensor]], steps: int, cls):
    """Per-step structs from the flat per-step tensors in module order (see MEFC_STEP_PARAMS); a host array of ``steps``."""
    arr = (cls * steps)()
    for t in range(steps):
        q = ts[t * MEFC_STEP_PARAMS:(t + 1) * MEFC_STEP_PARAMS]
        st = arr[t]
        for k in range(4):
            st.sep_dw1[k], st.sep_pw1[k], st.sep_dw2[k], st.sep_pw2[k] = (_p(v) for v in q[4 * k:4 * k + 4])
        for k in range(3):
            st.dil_dw[k], st.dil_pw[k] = _p(q[16 + 2 * k]), _p(q[17 + 2 * k])
        st.out_w = _p(q[22])
    return arr


def mefc_sizes(B: int, Cc: int, H: int, W: int, dtype: torch.dtype, steps: int) -> Tuple[int, int]:
    """(saved bytes, workspace bytes) of one MEFC layer pair; (0, 0) for a shape the kernels do not cover.  No GPU needed."""
    s = L.MefcShape(B, Cc, H, W, _dtype_code(dtype), int(steps))
    lib = L.lib()
    return int(lib.mi_mefc_saved_bytes(C.byref(s))), int(lib.mi_mefc_workspace(C.byref(s)))


def mefc_fwd(x: Tensor, params: Sequence[Tensor], steps: int, need_saved: bool):
    """One MEFC layer pair (OALayer routing + GroupOLs, DRSformer_arch.py:206-247, 346-351).  params = (ca_fc.0.weight, .bias,
    ca_fc.2.weight, .bias, preprocess.op.0.weight) + per step the 23 OperationLayer weights in module order.  -> (out, saved)."""
    _gpu(x, *params)
    for t in params[5:]:
        _f32(t, "MEFC parameter")
    if len(params) != 5 + MEFC_STEP_PARAMS * steps:
        raise ValueError(f"mefc: expected {5 + MEFC_STEP_PARAMS * steps} parameters for {steps} steps, got {len(params)}")
    s = _mefc_shape(x, steps)
    lib = L.lib()
    ws_bytes = lib.mi_mefc_workspace(C.byref(s))
    if ws_bytes == 0:
        L.check(-1, "mefc_workspace")
    out = torch.empty_like(x)
    saved = _blob(lib.mi_mefc_saved_bytes(C.byref(s)), x.device) if need_saved else None
    ws = _ws(ws_bytes, x.device)
    arr = _mefc_steps(params[5:], steps, L.MefcStepParams)
    pp = _f32_struct(L.MefcParams, params[:5], "MEFC parameter", C.cast(arr, C.POINTER(L.MefcStepParams)))
    L.check(lib.mi_mefc_fwd(C.byref(s), C.byref(pp), _p(x), _p(out), _p(saved), _p(ws), _stream()), "mefc_fwd")
    return out, saved


def mefc_saved_views(saved: Tensor, x: Tensor, steps: int) -> dict:
    """Views into a training forward's saved blob (mi_mefc_saved_bytes' layout): pooled [B, C], hpre [B, 16 steps] (fc1 output),
    w [B, steps, 8] (routing weights) in fp32, and per step lists s, d1, u, z, pre of x's dtype: the step input s_t [B, C, H, W],
    dw1 outputs [B, 4C, ..], pw1 outputs U [B, 4C, ..], Z [B, 8C, ..] and the out projection's pre-activation [B, C, ..]."""
    B, Cc, H, W = x.shape
    N = H * W
    off = [0]

    def take(n, dtype):
        es = torch.empty((), dtype=dtype).element_size()
        o = off[0]
        off[0] += (n * es + 255) // 256 * 256
        return saved[o:o + n * es].view(dtype)

    v = {"pooled": take(B * Cc, torch.float32).view(B, Cc), "hpre": take(B * 16 * steps, torch.float32).view(B, 16 * steps),
         "w": take(B * 8 * steps, torch.float32).view(B, steps, 8)}
    for name in ("s", "d1", "u", "z", "pre"):
        v[name] = []
    for _ in range(steps):
        for name, k in (("s", 1), ("d1", 4), ("u", 4), ("z", 8), ("pre", 1)):
            v[name].append(take(B * k * Cc * N, x.dtype).view(B, k * Cc, H, W))
        for _m in range(3):
            take(B * Cc * 8 * Cc, torch.float32 if _m == 0 else torch.bfloat16)
    return v


def mefc_bwd(x: Tensor, out: Tensor, dout: Tensor, params: Sequence[Tensor], steps: int, saved: Tensor,
             grads: Sequence[Tensor], accumulate: bool) -> Tensor:
    """Backward of mefc_fwd (``out``: its output): dx; the parameter gradients are written (accumulate: added) into ``grads``."""
    _gpu(x, out, dout, saved, *params, *grads)
    for t in grads[5:]:
        _f32(t, "MEFC gradient")
    s = _mefc_shape(x, steps)
    lib = L.lib()
    dx = torch.empty_like(x)
    pa = _mefc_steps(params[5:], steps, L.MefcStepParams)
    ga = _mefc_steps(grads[5:], steps, L.MefcStepGrads)
    pp = _f32_struct(L.MefcParams, params[:5], "MEFC parameter", C.cast(pa, C.POINTER(L.MefcStepParams)))
    gg = _f32_struct(L.MefcGrads, grads[:5], "MEFC gradient", C.cast(ga, C.POINTER(L.MefcStepGrads)), int(accumulate))
    ws = _ws(lib.mi_mefc_workspace(C.byref(s)), x.device)
    L.check(lib.mi_mefc_bwd(C.byref(s), C.byref(pp), _p(x), _p(out), _p(dout), _p(dx), C.byref(gg), _p(saved), _p(ws), _stream()),
            "mefc_bwd")
    return dx


def bwd_tail_ok(M: int, Cc: int, N: int, dtype: torch.dtype) -> bool:
    return bool(L.lib().mi_bwd_tail_ok(M, Cc, N, _dtype_code(dtype)))


BWD_TAIL_PLAN_FIELDS = ("covered", "pays", "waves", "fragments", "rows_per_wave", "mpad", "workgroups", "tiles", "passes",
                        "active_waves", "lds", "workspace")


def bwd_tail_plan(M: int, Cc: int, B: int, N: int, dtype: torch.dtype) -> dict:
    """What bwd_tail launches for dy [B, M, N] over x [B, Cc, N] under the current MI_BT_WIDE (mi_bwd_tail_plan; no GPU work).
    A shape the kernel does not cover gives covered = False and zeros."""
    out = (L.c_i64 * 12)()
    L.check(L.lib().mi_bwd_tail_plan(M, Cc, B, N, _dtype_code(dtype), out), "bwd_tail_plan")
    p = dict(zip(BWD_TAIL_PLAN_FIELDS, out))
    p["covered"], p["pays"] = bool(p["covered"]), bool(p["pays"])
    return p


def bwd_tail(dy: Tensor, x: Tensor, dres: Optional[Tensor], mean: Tensor, rstd: Tensor, w: Tensor, gamma: Tensor,
             beta: Tensor, dw: Tensor, dgamma: Tensor, dbeta: Tensor, accumulate: bool) -> Tensor:
    """The backward tail by itself (mi_bwd_tail): dy [B,M,H,W], x the LayerNorm input [B,C,H,W]; returns dx."""
    _gpu(dy, x, dres, mean, rstd, w, gamma, beta, dw, dgamma, dbeta)
    B, Cc, H, W = x.shape
    M = dy.shape[1]
    dx = torch.empty_like(x)
    lib = L.lib()
    ws = _ws(lib.mi_bwd_tail_workspace(M, Cc), x.device)
    L.check(lib.mi_bwd_tail(_p(dy), M, _p(x), Cc, _p(dres), _p(mean), _p(rstd), _p(w), _p(gamma), _p(beta), _p(dx), _p(dw),
                            _p(dgamma), _p(dbeta), B, H * W, int(accumulate), _dt(x), _p(ws), _stream()), "bwd_tail")
    return dx


# ----------------------------------------------------------------------------- fused half-blocks (bf16)
def _gdfn_fused_shape(x: Tensor, hidden: int, with_bias: bool) -> L.GdfnFusedShape:
    B, Cc, H, W = x.shape
    return L.GdfnFusedShape(B, Cc, hidden, H, W, int(with_bias))


def gdfn_fused_ok(x: Tensor, hidden: int, ks: int = 3) -> bool:
    """True when the one-launch LN + GDFN + residual kernel covers this activation (bf16, 3x3, tile-aligned)."""
    if x.dtype != torch.bfloat16 or ks != 3 or not x.is_cuda:
        return False
    s = _gdfn_fused_shape(x, hidden, True)
    return bool(L.lib().mi_gdfn_fused_ok(C.byref(s)))


def gdfn_fused_pack(x_like: Tensor, ln_w: Tensor, ln_b: Optional[Tensor], params: "GdfnParamsT") -> Tensor:
    """LayerNorm affine + GDFN parameters -> the fused kernel's packed weight images (re-run after weight updates)."""
    _gpu(ln_w, ln_b, *params)
    _f32(ln_w, "fused GDFN parameter"); _f32(ln_b, "fused GDFN parameter")
    hidden = params[4].shape[1]
    s = _gdfn_fused_shape(x_like, hidden, ln_b is not None)
    lib = L.lib()
    pack = _blob(lib.mi_gdfn_fused_pack_bytes(C.byref(s)), ln_w.device)
    pp = _f32_struct(L.GdfnParams, params, "fused GDFN parameter")
    L.check(lib.mi_gdfn_fused_pack(C.byref(s), _p(ln_w), _p(ln_b), C.byref(pp), _p(pack), _stream()), "gdfn_fused_pack")
    return pack


def gdfn_fused_fwd(y: Tensor, pack: Tensor, hidden: int, with_bias: bool, want_stats: bool = False,
                   f8: Optional[F8ScalesT] = None):
    """out = y + GDFN(LN(y)) in one launch; optionally the LN statistics [B, H*W] of y.  f8 = (x1, w1, x2, w2): fp8 e4m3 MFMA
    operands in both projections (inference: no statistics); x1 scales the normalised input, w1 the packed W_in . diag(gamma)."""
    _gpu(y, pack)
    s = _gdfn_fused_shape(y, hidden, with_bias)
    out = torch.empty_like(y)
    if f8 is not None:
        if want_stats:
            raise ValueError("fp8 projections are an inference path: no statistics")
        L.check(L.lib().mi_gdfn_fused_fwd_f8(C.byref(s), _p(pack), C.byref(L.F8Scales(*[float(v) for v in f8])), _p(y), _p(out),
                                             _stream()), "gdfn_fused_fwd_f8")
        return out, None, None
    mean = rstd = None
    if want_stats:
        mean = torch.empty((y.shape[0], y.shape[2] * y.shape[3]), dtype=torch.float32, device=y.device)
        rstd = torch.empty_like(mean)
    L.check(L.lib().mi_gdfn_fused_fwd(C.byref(s), _p(pack), _p(y), _p(out), _p(mean), _p(rstd), _stream()), "gdfn_fused_fwd")
    return out, mean, rstd


GDFN_FUSED_ENTRIES = ("inference", "train", "f8")
GDFN_FUSED_PLAN_FIELDS = ("covered", "family", "C", "th", "tw", "pc", "waves", "save", "f8", "nch", "ngr", "tiles_x", "tiles_y", "S",
                          "grid", "block", "lds", "xcd_pairs", "pack_bytes", "pack_pc")


def gdfn_fused_plan(shape, hidden: int, entry: str = "inference", with_bias: bool = True) -> dict:
    """What gdfn_fused_fwd ("inference"), gdfn_fused_fwd_train ("train") or the fp8 form ("f8") launches for a [B, C, H, W]
    activation under the current MI_FG_CFG / MI_FG_NOXCD (mi_gdfn_fused_plan; no GPU work).  family is "tile" or "fourth";
    pack_pc is the chunk width gdfn_fused_pack builds the pack for: pack and run under the same switches.  An entry with no
    kernel instance gives covered = False and zeros."""
    B, Cc, H, W = shape
    out = (L.c_i64 * 20)()
    s = L.GdfnFusedShape(B, Cc, hidden, H, W, int(with_bias))
    L.check(L.lib().mi_gdfn_fused_plan(C.byref(s), GDFN_FUSED_ENTRIES.index(entry), out), "gdfn_fused_plan")
    p = dict(zip(GDFN_FUSED_PLAN_FIELDS, out))
    for k in ("covered", "save", "f8", "xcd_pairs"):
        p[k] = bool(p[k])
    p["family"] = ("tile", "fourth")[p["family"]] if p["covered"] else None
    return p


MDTA_FUSED_PLAN_FIELDS = ("covered", "pays", "kind", "form", "th", "tiles_x", "tiles_y", "S", "grid", "block", "lds", "part_mult",
                          "part_bytes", "workspace", "pack_bytes", "waves")


def mdta_fused_plan(shape, heads: int, ks: int = 3, dtype: torch.dtype = torch.bfloat16) -> dict:
    """What pass A of mdta_fused_fwd launches for a [B, C, H, W] activation under the current MI_FM_CFG (mi_mdta_fused_plan; no
    GPU work).  kind is "48_1", "96_2" or "96_1" (C, heads), form "round3" or "fourth".  A shape the kernel does not cover gives
    covered = False and zeros."""
    B, Cc, H, W = shape
    out = (L.c_i64 * 16)()
    s = L.MdtaShape(B, Cc, heads, H, W, _dtype_code(dtype), ks)
    L.check(L.lib().mi_mdta_fused_plan(C.byref(s), out), "mdta_fused_plan")
    p = dict(zip(MDTA_FUSED_PLAN_FIELDS, out))
    p["covered"], p["pays"] = bool(p["covered"]), bool(p["pays"])
    p["kind"] = (None, "48_1", "96_2", "96_1")[p["kind"]]
    p["form"] = ("round3", "fourth")[p["form"]] if p["covered"] else None
    return p


def gdfn_fused_train_ok(x: Tensor, hidden: int, ks: int = 3) -> bool:
    """True when the one-launch LN + GDFN forward can also write what the backward reads (mi_gdfn_fused_fwd_train)."""
    if x.dtype != torch.bfloat16 or ks != 3 or not x.is_cuda:
        return False
    return bool(L.lib().mi_gdfn_fused_fwd_train_ok(C.byref(_gdfn_fused_shape(x, hidden, True))))


def gdfn_fused_fwd_train(y: Tensor, pack: Tensor, hidden: int, with_bias: bool):
    """out = y + GDFN(LN(y)) in one launch on the TRAINING path -> (out, saved, mean, rstd): ``saved`` is the blob gdfn_bwd
    reads (project_in output + gate output), mean / rstd the LayerNorm statistics of y."""
    _gpu(y, pack)
    s = _gdfn_fused_shape(y, hidden, with_bias)
    lib = L.lib()
    out = torch.empty_like(y)
    mean = torch.empty((y.shape[0], y.shape[2] * y.shape[3]), dtype=torch.float32, device=y.device)
    rstd = torch.empty_like(mean)
    saved = _blob(lib.mi_gdfn_saved_bytes(C.byref(_gdfn_shape(y, hidden, 3, 0))), y.device)
    L.check(lib.mi_gdfn_fused_fwd_train(C.byref(s), _p(pack), _p(y), _p(out), _p(mean), _p(rstd), _p(saved), _stream()),
            "gdfn_fused_fwd_train")
    return out, saved, mean, rstd


def mdta_fused_ok(x: Tensor, heads: int, ks: int = 3) -> bool:
    """True when the one-launch LN -> qkv -> dw3x3 -> q k^T pass (csrc/fused_mdta.hip) covers this activation."""
    if x.dtype != torch.bfloat16 or ks != 3 or not x.is_cuda:
        return False
    return bool(L.lib().mi_mdta_fused_ok(C.byref(_mdta_shape(x, heads, ks))))


def mdta_fused_pays(x: Tensor, heads: int, ks: int = 3) -> bool:
    """Covered and large enough (one workgroup for nearly every CU) for the fused pass to beat the unfused chain."""
    if x.dtype != torch.bfloat16 or ks != 3 or not x.is_cuda:
        return False
    return bool(L.lib().mi_mdta_fused_pays(C.byref(_mdta_shape(x, heads, ks))))


def mdta_fused_pack(x_like: Tensor, heads: int, ln_w: Tensor, ln_b: Optional[Tensor], params: "MdtaParamsT") -> Tensor:
    """LayerNorm affine + qkv / depthwise parameters -> the fused MDTA kernel's packed weight images."""
    _gpu(ln_w, ln_b, *params)
    _f32(ln_w, "fused MDTA parameter"); _f32(ln_b, "fused MDTA parameter")
    s = _mdta_shape(x_like, heads, params[3].shape[-1])
    lib = L.lib()
    pack = _blob(lib.mi_mdta_fused_pack_bytes(C.byref(s)), ln_w.device)
    L.check(lib.mi_mdta_fused_pack(C.byref(s), _p(ln_w), _p(ln_b), C.byref(_mdta_params(params)), _p(pack), _stream()),
            "mdta_fused_pack")
    return pack


def mdta_fused_fwd(x: Tensor, pack: Tensor, params: "MdtaParamsT", heads: int, with_bias: bool, residual: Optional[Tensor],
                   want_stats: bool = False):
    """out = residual + MDTA(LN(x)) with the whole producer chain of q k^T in one launch (nothing saved: the no_grad path).
    -> (out, mean, rstd)."""
    _gpu(x, pack, residual, *params)
    s = _mdta_shape(x, heads, params[3].shape[-1])
    lib = L.lib()
    out = torch.empty_like(x)
    mean = rstd = None
    if want_stats:
        mean = torch.empty((x.shape[0], x.shape[2] * x.shape[3]), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
    ws = _ws(lib.mi_mdta_fused_workspace(C.byref(s)), x.device)
    L.check(lib.mi_mdta_fused_fwd(C.byref(s), C.byref(_mdta_params(params)), _p(pack), int(with_bias), _p(x), _p(residual),
                                  _p(out), _p(mean), _p(rstd), _p(ws), _stream()), "mdta_fused_fwd")
    return out, mean, rstd


# ----------------------------------------------------------------------------- router GAP
def rows_gather(x: Tensor, idx: Tensor) -> Tensor:
    """out[i] = x[idx[i]] over whole [C,H,W] rows (SparseDispatcher.dispatch)."""
    _gpu(x, idx)
    assert idx.dtype == torch.int64 and x.is_contiguous()
    n = int(idx.numel())
    out = torch.empty((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    row = x[0].numel()
    L.check(L.lib().mi_rows_gather(_p(x), _p(idx), _p(out), n, row, _dt(x), _stream()), "rows_gather")
    return out


def rows_gather_scaled(x_f32: Tensor, idx: Tensor, scale: Optional[Tensor], dtype: torch.dtype) -> Tensor:
    """out[i] = scale[i] * x_f32[idx[i]] cast to `dtype`."""
    _gpu(x_f32, idx, scale)
    assert x_f32.dtype == torch.float32 and idx.dtype == torch.int64 and x_f32.is_contiguous()
    n = int(idx.numel())
    out = torch.empty((n,) + tuple(x_f32.shape[1:]), dtype=dtype, device=x_f32.device)
    L.check(L.lib().mi_rows_gather_scaled(_p(x_f32), _p(idx), _p(_f32(scale, "scale")), _p(out), n, x_f32[0].numel(),
                                          _dtype_code(dtype), _stream()), "rows_gather_scaled")
    return out


def rows_scatter_add(src: Tensor, idx: Tensor, scale: Optional[Tensor], n_rows: int, out_f32: bool) -> Tensor:
    """out[b] = sum_{i: idx[i]==b} scale[i] * src[i], accumulated in fp32 (SparseDispatcher.combine)."""
    _gpu(src, idx, scale)
    assert idx.dtype == torch.int64 and src.is_contiguous()
    out = torch.empty((n_rows,) + tuple(src.shape[1:]), dtype=torch.float32 if out_f32 else src.dtype, device=src.device)
    row = src[0].numel() if src.shape[0] else out[0].numel()
    L.check(L.lib().mi_rows_scatter_add(_p(src), _p(idx), _p(_f32(scale, "scale")), _p(out), int(src.shape[0]), n_rows, row,
                                        _dt(src), 1 if out_f32 else 0, _stream()), "rows_scatter_add")
    return out


def rows_dot(g: Tensor, src: Tensor, idx: Tensor) -> Tensor:
    """out[i] = <g[idx[i]], src[i]> (fp32 g): gradient of the combine's gate values."""
    _gpu(g, src, idx)
    n = int(src.shape[0])
    out = torch.zeros(n, dtype=torch.float32, device=src.device)
    if n == 0:
        return out
    row = src[0].numel()
    ws = _ws(L.lib().mi_rows_dot_workspace(n, row), src.device)
    L.check(L.lib().mi_rows_dot(_p(_f32(g, "g")), _p(src), _p(idx), _p(out), n, row, _dt(src), _p(ws), _stream()), "rows_dot")
    return out


def glue3x3_ok(H: int, W: int) -> bool:
    return bool(L.lib().mi_glue3x3_ok(H, W))


def im2col3x3(x: Tensor, flip: bool = False) -> Tensor:
    """x[B,C,H,W] -> [B,9C,H,W] with col[c*9+ky*3+kx][y][x] = x[c][y+ky-1][x+kx-1] (shifts negated when flip)."""
    _gpu(x)
    B, Cn, H, W = x.shape
    out = torch.empty((B, 9 * Cn, H, W), dtype=x.dtype, device=x.device)
    L.check(L.lib().mi_im2col3x3(_p(x), _p(out), B, Cn, H, W, 1 if flip else 0, _dt(x), _stream()), "im2col3x3")
    return out


def col2im3x3(z: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None, flip: bool = False) -> Tensor:
    """z[B,9M,H,W] -> y[B,M,H,W], y[m] = sum over taps of the tap plane shifted back (+ bias[m]) (+ residual);
    flip negates the shifts (transposed convolution)."""
    _gpu(z, bias, residual)
    B, M9, H, W = z.shape
    M = M9 // 9
    y = torch.empty((B, M, H, W), dtype=z.dtype, device=z.device)
    L.check(L.lib().mi_col2im3x3(_p(z), _p(_f32(bias, "bias")), _p(residual), _p(y), B, M, H, W, 1 if flip else 0, _dt(z), _stream()), "col2im3x3")
    return y


GLUE3X3_PLAN_FIELDS = ("fast", "lpr", "band", "bands", "blocks_im2col", "blocks_col2im")


def glue3x3_plan(planes: int, H: int, W: int, dtype: torch.dtype, aligned: bool = True) -> dict:
    """What im2col3x3 / col2im3x3 launch for `planes` planes (B * C, B * M) of H x W whose pointers all are / are not on a 16-byte
    boundary (mi_glue3x3_plan; no GPU work)."""
    out = (L.c_i64 * 6)()
    L.check(L.lib().mi_glue3x3_plan(planes, H, W, _dtype_code(dtype), int(aligned), out), "glue3x3_plan")
    p = dict(zip(GLUE3X3_PLAN_FIELDS, out))
    p["fast"] = bool(p["fast"])
    return p


def chan_sum(x: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """Bias gradient of a conv: out[c] (+)= sum over batch and pixels of x[b, c] (fp32, fixed order)."""
    _gpu(x, out)
    B, Cn, H, W = x.shape
    if out is None:
        if accumulate:
            raise ValueError("chan_sum: accumulate needs the gradient buffer")
        out = torch.empty(Cn, dtype=torch.float32, device=x.device)
    _f32(out, "bias gradient")
    lib = L.lib()
    ws = _ws(lib.mi_chan_sum_workspace(Cn, H * W), x.device)
    L.check(lib.mi_chan_sum(_p(x), _p(out), B, Cn, H * W, _dt(x), 1 if accumulate else 0, _p(ws), _stream()), "chan_sum")
    return out


CHAN_SUM_PLAN_FIELDS = ("splits", "per_split", "vector", "workspace")


def chan_sum_plan(B: int, Cn: int, N: int, dtype: torch.dtype, aligned: bool = True) -> dict:
    """What chan_sum launches for x [B, Cn, N] whose base pointer is / is not on a 16-byte boundary (mi_chan_sum_plan; no GPU
    work)."""
    out = (L.c_i64 * 4)()
    L.check(L.lib().mi_chan_sum_plan(B, Cn, N, _dtype_code(dtype), int(aligned), out), "chan_sum_plan")
    p = dict(zip(CHAN_SUM_PLAN_FIELDS, out))
    p["vector"] = bool(p["vector"])
    return p


ATTN_SMALL_PLAN_FIELDS = ("instance", "promoted", "padded", "rpw", "fold_grid_x", "fold_grid_y", "last_chunks", "fold_lds",
                          "fold_raised", "bwd_grid_x", "bwd_grid_y", "bwd_lds", "bwd_raised", "row_blocks", "mtb_vector",
                          "wd_vector")


def attn_small_plan(B: int, Cn: int, heads: int) -> dict:
    """What the c x c side of MDTA launches for B images of Cn channels in `heads` heads (mi_attn_small_plan; no GPU work)."""
    out = (L.c_i64 * 16)()
    L.check(L.lib().mi_attn_small_plan(B, Cn, heads, out), "attn_small_plan")
    p = dict(zip(ATTN_SMALL_PLAN_FIELDS, out))
    for k in ("promoted", "fold_raised", "bwd_raised", "mtb_vector", "wd_vector"):
        p[k] = bool(p[k])
    return p


def _attn_small_out(out: Optional[dict], name: str, shape, dtype, device, want: bool = True) -> Optional[Tensor]:
    if out is not None:
        t = out.get(name)
        if t is not None and (tuple(t.shape) != tuple(shape) or t.dtype != dtype):
            raise ValueError(f"attn_small: {name} must be {tuple(shape)} of {dtype}")
        return t
    return torch.empty(shape, dtype=dtype, device=device) if want else None


def attn_small_fwd(graw: Tensor, ss: Tensor, temperature: Tensor, wo: Tensor, heads: int, mb: bool = True, mtb: bool = True,
                   out: Optional[dict] = None) -> dict:
    """The attention fold by itself (mi_attn_small_fwd): graw [Z,c,c], ss [Z,2c], temperature [heads], wo [C,C], all fp32.
    Returns P, A [Z,c,c], nrm [Z,2c], M [B,C,C] (fp32) and the bf16 Mb = M, Mtb = M^T per image (None when not asked for).
    out: the caller's buffers by these names instead (Mb / Mtb absent: not written)."""
    Cn, c = wo.shape[0], wo.shape[0] // heads
    Z = graw.shape[0]
    B = Z // heads
    f32, b16, dev = torch.float32, torch.bfloat16, graw.device
    o = {"P": _attn_small_out(out, "P", (Z, c, c), f32, dev), "A": _attn_small_out(out, "A", (Z, c, c), f32, dev),
         "nrm": _attn_small_out(out, "nrm", (Z, 2 * c), f32, dev), "M": _attn_small_out(out, "M", (B, Cn, Cn), f32, dev),
         "Mb": _attn_small_out(out, "Mb", (B, Cn, Cn), b16, dev, mb), "Mtb": _attn_small_out(out, "Mtb", (B, Cn, Cn), b16, dev, mtb)}
    _gpu(graw, ss, temperature, wo, *o.values())
    for t, what in ((graw, "graw"), (ss, "ss"), (temperature, "temperature"), (wo, "wo")):
        _f32(t, what)
    if tuple(graw.shape) != (B * heads, c, c) or tuple(ss.shape) != (Z, 2 * c) or tuple(wo.shape) != (Cn, Cn) or temperature.numel() != heads:
        raise ValueError("attn_small_fwd: graw [B heads, c, c], ss [B heads, 2c], temperature [heads], wo [C, C] with c = C / heads")
    L.check(L.lib().mi_attn_small_fwd(_p(graw), _p(ss), _p(temperature), _p(wo), _p(o["P"]), _p(o["A"]), _p(o["nrm"]), _p(o["M"]),
                                      _p(o["Mb"]), _p(o["Mtb"]), B, Cn, heads, _stream()), "attn_small_fwd")
    return o


def attn_small_bwd(dM: Tensor, A: Tensor, P: Tensor, nrm: Tensor, temperature: Tensor, wo: Tensor, heads: int, wdb: bool = True,
                   out: Optional[dict] = None) -> dict:
    """The attention backward's c x c side by itself (mi_attn_small_bwd): dM [B,C,C] and the forward's A, P, nrm.  Returns
    dwo_part [B,C,C], dtemp_part [Z], wd [Z,2c,2c] (fp32) and the bf16 wdb = wd (None when not asked for).  out: as in
    attn_small_fwd."""
    B, Cn = dM.shape[0], dM.shape[1]
    c, Z = Cn // heads, B * heads
    f32, dev = torch.float32, dM.device
    o = {"dwo_part": _attn_small_out(out, "dwo_part", (B, Cn, Cn), f32, dev), "dtemp_part": _attn_small_out(out, "dtemp_part", (Z,), f32, dev),
         "wd": _attn_small_out(out, "wd", (Z, 2 * c, 2 * c), f32, dev),
         "wdb": _attn_small_out(out, "wdb", (Z, 2 * c, 2 * c), torch.bfloat16, dev, wdb)}
    _gpu(dM, A, P, nrm, temperature, wo, *o.values())
    for t, what in ((dM, "dM"), (A, "A"), (P, "P"), (nrm, "nrm"), (temperature, "temperature"), (wo, "wo")):
        _f32(t, what)
    if (tuple(dM.shape) != (B, Cn, Cn) or tuple(A.shape) != (Z, c, c) or tuple(P.shape) != (Z, c, c) or tuple(nrm.shape) != (Z, 2 * c)
            or tuple(wo.shape) != (Cn, Cn) or temperature.numel() != heads):
        raise ValueError("attn_small_bwd: dM [B, C, C], A, P [B heads, c, c], nrm [B heads, 2c], temperature [heads], wo [C, C]")
    L.check(L.lib().mi_attn_small_bwd(_p(dM), _p(A), _p(P), _p(nrm), _p(temperature), _p(wo), _p(o["dwo_part"]), _p(o["dtemp_part"]),
                                      _p(o["wd"]), _p(o["wdb"]), B, Cn, heads, _stream()), "attn_small_bwd")
    return o


def conv3x3_ok(x: Tensor) -> bool:
    """The implicit-GEMM 3x3 convolution covers this activation (bf16, W % 8 == 0; csrc/conv3x3.hip)."""
    return bool(x.is_cuda and x.dim() == 4 and L.lib().mi_conv3x3_ok(x.shape[2], x.shape[3], _dt(x)))


def conv3x3(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
            transpose: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """Dense 3x3 conv (stride 1, pad 1) of x [B,K,H,W] as an implicit GEMM.  transpose False: weight [M,K,3,3], y = conv(x).
    transpose True: weight is the conv's own [K,M,3,3] and the result is its data gradient for the upstream gradient x.
    x / residual / out may be channel slices (dense [C,H,W] blocks, any batch stride)."""
    _gpu(weight, bias)
    for tsr in (x, residual, out):                       # channel slices allowed: checked for dense [C,H,W] blocks below
        if tsr is not None and not tsr.is_cuda:
            raise RuntimeError("image_restoration_amd ops run on the MI355X only (got a CPU tensor)")
    _f32(weight, "conv weight")
    B, K, H, W = x.shape
    M = weight.shape[1] if transpose else weight.shape[0]
    if (weight.shape[0] if transpose else weight.shape[1]) != K or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"conv3x3: weight {tuple(weight.shape)} does not match {K} input channels")
    for tsr, name in ((x, "x"), (residual, "residual"), (out, "out")):
        if tsr is not None and not (tsr.stride(3) == 1 and tsr.stride(2) == W and tsr.stride(1) == H * W):
            raise ValueError(f"conv3x3: {name} must have dense [C,H,W] blocks")
    lib = L.lib()
    w = weight.contiguous()
    pack = _blob(lib.mi_conv3x3_pack_bytes(M, K), x.device)
    L.check(lib.mi_conv3x3_pack(_p(w), M, K, 1 if transpose else 0, _p(pack), _stream()), "conv3x3_pack")
    y = out if out is not None else torch.empty((B, M, H, W), dtype=x.dtype, device=x.device)
    L.check(lib.mi_conv3x3_fwd(_p(pack), _p(x), x.stride(0), _p(_f32(bias, "bias")), _p(residual),
                               residual.stride(0) if residual is not None else 0, _p(y), y.stride(0), B, M, K, H, W, _stream()),
            "conv3x3_fwd")
    return y


def conv3x3_wgrad(dy: Tensor, x: Tensor, dw: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """Weight gradient of the dense 3x3 conv: dw[M,K,3,3] (+)= sum over batch and pixels of dy[b,m,p] x[b,k,p+d(tap)] without the
    im2col expansion.  dy [B,M,H,W], x [B,K,H,W] bf16 (channel slices allowed); dw fp32 (allocated when None)."""
    _gpu(dw)
    for tsr, name in ((dy, "dy"), (x, "x")):
        if not tsr.is_cuda:
            raise RuntimeError("image_restoration_amd ops run on the MI355X only (got a CPU tensor)")
        if not (tsr.stride(3) == 1 and tsr.stride(2) == tsr.shape[3] and tsr.stride(1) == tsr.shape[2] * tsr.shape[3]):
            raise ValueError(f"conv3x3_wgrad: {name} must have dense [C,H,W] blocks")
    B, M, H, W = dy.shape
    K = x.shape[1]
    if dw is None:
        if accumulate:
            raise ValueError("conv3x3_wgrad: accumulate needs the gradient buffer")
        dw = torch.empty((M, K, 3, 3), dtype=torch.float32, device=dy.device)
    _f32(dw, "conv weight gradient")
    lib = L.lib()
    ws = _ws(lib.mi_conv3x3_wgrad_workspace(B, M, K, H, W), dy.device)
    L.check(lib.mi_conv3x3_wgrad(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(dw), 1 if accumulate else 0, B, M, K, H, W, _p(ws),
                                 _stream()), "conv3x3_wgrad")
    return dw


def pixel_shuffle2(x: Tensor, unshuffle: bool, out: Optional[Tensor] = None) -> Tensor:
    """PixelShuffle(2) (unshuffle False: [B,4c,H,W] -> [B,c,2H,2W]) or its inverse.  x / out may be channel slices of wider
    tensors (dense [C,H,W] blocks, any batch stride)."""
    if not x.is_cuda:
        raise RuntimeError("image_restoration_amd ops run on the MI355X only (got a CPU tensor)")
    B, Cx, Hx, Wx = x.shape
    if unshuffle:
        c, H, W = Cx, Hx // 2, Wx // 2
        shape = (B, 4 * c, H, W)
    else:
        c, H, W = Cx // 4, Hx, Wx
        shape = (B, c, 2 * H, 2 * W)
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    assert tuple(out.shape) == shape and out.dtype == x.dtype
    L.check(L.lib().mi_pixel_shuffle2(_p(x), _bstride(x), _p(out), _bstride(out), B, c, H, W, int(unshuffle), _dt(x), _stream()),
            "pixel_shuffle2")
    return out


def copy_rows(src: Tensor, dst: Tensor) -> Tensor:
    """dst <- src for [B,C,H,W] tensors whose [C,H,W] blocks are dense (either may be a channel slice)."""
    B = src.shape[0]
    L.check(L.lib().mi_copy_rows(_p(src), _bstride(src), _p(dst), _bstride(dst), B, src[0].numel(), _dt(src), _stream()), "copy_rows")
    return dst


CONV3X3_PLAN_FIELDS = ("mt", "twp", "tr", "tiles_x", "tiles_y", "co_tiles", "chunks", "pack_bytes", "w_swap", "w_rows", "w_cols",
                       "w_splits", "w_grid_x", "w_grid_y", "w_workspace")
VEC_PLAN_FIELDS = ("vector", "total", "blocks")


def conv3x3_plan(B: int, M: int, K: int, H: int, W: int) -> dict:
    """What conv3x3 (M planes written, K read: for the data gradient pass them as that call sees them) and conv3x3_wgrad launch
    for a [B, K, H, W] bf16 input (mi_conv3x3_plan; no GPU work)."""
    out = (L.c_i64 * 15)()
    L.check(L.lib().mi_conv3x3_plan(B, M, K, H, W, out), "conv3x3_plan")
    p = dict(zip(CONV3X3_PLAN_FIELDS, out))
    p["w_swap"] = bool(p["w_swap"])
    return p


def pixel_shuffle2_plan(B: int, c: int, H: int, W: int, in_bs: int, out_bs: int, dtype: torch.dtype, aligned: bool = True) -> dict:
    """What pixel_shuffle2 launches; c, H, W are the low-resolution side's, the batch strides in elements (0 = dense)
    (mi_pixel_shuffle2_plan; no GPU work)."""
    out = (L.c_i64 * 3)()
    L.check(L.lib().mi_pixel_shuffle2_plan(B, c, H, W, in_bs, out_bs, _dtype_code(dtype), int(aligned), out), "pixel_shuffle2_plan")
    return dict(zip(VEC_PLAN_FIELDS, out))


def copy_rows_plan(rows: int, Ln: int, src_rs: int, dst_rs: int, dtype: torch.dtype, aligned: bool = True) -> dict:
    """What copy_rows launches for [rows][Ln] with row strides in elements (0 = Ln) (mi_copy_rows_plan; no GPU work)."""
    out = (L.c_i64 * 3)()
    L.check(L.lib().mi_copy_rows_plan(rows, Ln, src_rs, dst_rs, _dtype_code(dtype), int(aligned), out), "copy_rows_plan")
    return dict(zip(VEC_PLAN_FIELDS, out))


def gap_fwd(x: Tensor) -> Tensor:
    _gpu(x)
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    L.check(L.lib().mi_gap_fwd(_p(x), _p(out), B, Cc, H * W, _dt(x), _stream()), "gap_fwd")
    return out


def gap_bwd(dout: Tensor, like: Tensor) -> Tensor:
    dout = dout.contiguous()
    _gpu(dout, like)
    B, Cc, H, W = like.shape
    dx = torch.empty_like(like)
    L.check(L.lib().mi_gap_bwd(_p(dout.contiguous().float()), _p(dx), B, Cc, H * W, _dt(like), _stream()), "gap_bwd")
    return dx


# ----------------------------------------------------------------------------- MoCE kernels (csrc/moce.hip)
class RouteTables:
    """Device-side SparseDispatcher bookkeeping produced by the router launch (no nonzero / sort / tolist)."""
    __slots__ = ("counts", "offsets", "perm", "perm_gate", "perm_expert", "row_of", "logits")


def moe_route_fwd(pooled: Tensor, freq: Tensor, wg: Tensor, wf: Tensor, noise: Tensor, complexity: Optional[Tensor], k: int,
                  training: bool):
    """-> gates [B,E], topk_idx [B,k] int64, topk_val [B,k], aux [1], RouteTables."""
    _gpu(pooled, freq, wg, wf, noise, complexity)
    for t in (pooled, freq, wg, wf, noise, complexity):
        _f32(t, "router tensor")
    B, Cc = pooled.shape
    Fd, E = freq.shape[1], wg.shape[0]
    dev = pooled.device
    f32 = dict(dtype=torch.float32, device=dev)
    gates, aux = torch.empty((B, E), **f32), torch.empty(1, **f32)
    idx = torch.empty((B, k), dtype=torch.int64, device=dev)
    val = torch.empty((B, k), **f32)
    tb = RouteTables()
    tb.logits = torch.empty((B, E), **f32)
    tb.counts = torch.empty(E, dtype=torch.int32, device=dev)
    tb.offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
    tb.perm = torch.empty(B * k, dtype=torch.int64, device=dev)
    tb.perm_gate = torch.empty(B * k, **f32)
    tb.perm_expert = torch.empty(B * k, dtype=torch.int32, device=dev)
    tb.row_of = torch.empty((B, k), dtype=torch.int32, device=dev)
    L.check(L.lib().mi_moe_route_fwd(_p(pooled), _p(freq), _p(wg), _p(wf), _p(noise), _p(complexity), _p(tb.logits), _p(gates),
                                     _p(idx), _p(val), _p(aux), _p(tb.counts), _p(tb.offsets), _p(tb.perm), _p(tb.perm_gate),
                                     _p(tb.perm_expert), _p(tb.row_of), B, Cc, Fd, E, k, int(training), _stream()),
            "moe_route_fwd")
    return gates, idx, val, aux, tb


def moe_route_bwd(pooled: Tensor, freq: Tensor, wg: Tensor, wf: Tensor, noise: Tensor, complexity: Optional[Tensor],
                  tb: RouteTables, idx: Tensor, dgates: Optional[Tensor], drow: Optional[Tensor], daux: Optional[Tensor],
                  training: bool):
    _gpu(pooled, freq, wg, wf, noise, complexity, dgates, drow, daux)
    B, Cc = pooled.shape
    Fd, E, k = freq.shape[1], wg.shape[0], idx.shape[1]
    dpooled, dfreq, dwg, dwf = (torch.empty_like(t) for t in (pooled, freq, wg, wf))
    L.check(L.lib().mi_moe_route_bwd(_p(pooled), _p(freq), _p(wg), _p(wf), _p(noise), _p(complexity), _p(tb.logits), _p(idx),
                                     _p(_f32(dgates, "dgates")), _p(_f32(drow, "drow")), _p(tb.row_of), _p(_f32(daux, "daux")),
                                     _p(dpooled), _p(dfreq), _p(dwg), _p(dwf), B, Cc, Fd, E, k, int(training), _stream()),
            "moe_route_bwd")
    return dpooled, dfreq, dwg, dwf


def grouped_pw_gemm(problems, counts: Tensor, offsets: Tensor, max_rows: int, n_pix: int, dtype: torch.dtype) -> None:
    """ONE launch for the 1x1 projections of all experts (csrc/grouped.hip).  ``problems``: list of dicts with keys
    x, w (2-D fp32 [M, K] or, with transposed=True, [K, M] used as its transpose), y, m, k, expert and optionally bias, r,
    x_local / y_local / r_local (the buffer is indexed by the row's position inside its expert's segment instead of the
    stitched row number).  counts / offsets: the router's int32 DEVICE tables - no segment size is read by the host here."""
    _gpu(counts, offsets)
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int32
    arr = (L.GroupedProblem * len(problems))()
    for i, q in enumerate(problems):
        w = q["w"]
        _f32(w, "expert weight")
        g = arr[i]
        g.x, g.x_rs = q["x"].data_ptr(), int(q.get("x_rs", 0))
        g.w = w.data_ptr()
        g.w_sm, g.w_sk = (1, w.stride(0)) if q.get("transposed") else (w.stride(0), 1)
        g.bias = _p(q.get("bias"))
        g.r, g.r_rs = _p(q.get("r")), int(q.get("r_rs", 0))
        g.y, g.y_rs = q["y"].data_ptr(), int(q.get("y_rs", 0))
        g.m, g.k, g.expert = int(q["m"]), int(q["k"]), int(q["expert"])
        g.x_local, g.y_local, g.r_local = int(bool(q.get("x_local"))), int(bool(q.get("y_local"))), int(bool(q.get("r_local")))
    L.check(L.lib().mi_grouped_pw_gemm(arr, len(problems), _p(counts), _p(offsets), int(max_rows), int(n_pix),
                                       _dtype_code(dtype), _stream()), "grouped_pw_gemm")


def _bstride(t: Tensor) -> int:
    """Batch stride (elements) of a [B,C,H,W] tensor whose [C,H,W] block is dense (a channel slice of a wider tensor)."""
    B, Cc, H, W = t.shape
    assert t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W, "need dense [C,H,W] blocks"
    return t.stride(0) if B > 1 else Cc * H * W


def patch_circconv(x: Tensor, y: Tensor, patch: int, flip: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """Per patch x patch block: irfft2(rfft2(x) * rfft2(y)) = 2-D circular convolution (zero padded to the patch grid).
    x, y: [B,C,H,W] (channel slices allowed); flip convolves with the index-reversed y (gradient form)."""
    for t in (x, y):
        if not t.is_cuda:
            raise RuntimeError("image_restoration_amd ops run on the MI355X only (got a CPU tensor)")
    B, Cc, H, W = x.shape
    assert x.shape == y.shape and x.dtype == y.dtype
    if out is None:
        out = torch.empty((B, Cc, H, W), dtype=x.dtype, device=x.device)
    L.check(L.lib().mi_patch_circconv(_p(x), _bstride(x), _p(y), _bstride(y), _p(out), _bstride(out), B, Cc, H, W, int(patch),
                                      int(flip), _dt(x), _stream()), "patch_circconv")
    return out


def gelu_gap_fwd(x: Tensor) -> Tensor:
    _gpu(x)
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    L.check(L.lib().mi_gelu_gap_fwd(_p(x), _p(out), B, Cc, H * W, _dt(x), _stream()), "gelu_gap_fwd")
    return out


def gelu_gap_bwd(x: Tensor, dout: Tensor) -> Tensor:
    dout = dout.contiguous()
    _gpu(x, dout)
    B, Cc, H, W = x.shape
    dx = torch.empty_like(x)
    L.check(L.lib().mi_gelu_gap_bwd(_p(x), _p(dout.contiguous().float()), _p(dx), B, Cc, H * W, _dt(x), _stream()), "gelu_gap_bwd")
    return dx


def ewise_fwd(a: Tensor, b: Tensor, op: int) -> Tensor:
    """op 0: a * b ; op 1: a * silu(b).  a, b: [B,C,H,W], channel slices allowed."""
    B = a.shape[0]
    Ln = a[0].numel()
    out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    L.check(L.lib().mi_ewise_fwd(_p(a), _bstride(a), _p(b), _bstride(b), _p(out), B, Ln, op, _dt(a), _stream()), "ewise_fwd")
    return out


def ewise_bwd(a: Tensor, b: Tensor, dout: Tensor, op: int, da: Optional[Tensor] = None, db: Optional[Tensor] = None):
    """Gradients of ewise_fwd; da / db may be given as (channel-slice) views to be written in place."""
    _gpu(dout)
    B = a.shape[0]
    Ln = a[0].numel()
    if da is None:
        da = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    if db is None:
        db = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    L.check(L.lib().mi_ewise_bwd(_p(a), _bstride(a), _p(b), _bstride(b), _p(dout), _p(da), _bstride(da), _p(db), _bstride(db), B,
                                 Ln, op, _dt(a), _stream()), "ewise_bwd")
    return da, db


# ----------------------------------------------------------------------------- training-step tail
def adamw_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, step: int, betas=(0.9, 0.999), eps: float = 1e-8,
               weight_decay: float = 1e-2, grad_scale: float = 1.0, dev_scalars: Optional[Tensor] = None) -> None:
    """dev_scalars: optional device tensor [lr, 1-b1^t, sqrt(1-b2^t)] that overrides lr/step (graph replay)."""
    _gpu(p, g, m, v, dev_scalars)
    L.check(L.lib().mi_adamw_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay, step,
                                  grad_scale, _p(dev_scalars), _stream()), "adamw_step")


def grad_sumsq_workspace(n: int, device) -> Tensor:
    """Device scratch for grad_sumsq over ``n`` elements (one fp64 partial per block)."""
    return _blob(L.lib().mi_grad_sumsq_workspace(int(n)), device)


def grad_sumsq(x: Tensor, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """Sum of squares of a flat fp32 buffer into a 1-element device tensor (bitwise reproducible, fp64 accumulation); no host
    sync.  ``out`` / ``workspace`` may be passed to keep their addresses fixed (graph capture)."""
    _gpu(x, out, workspace)
    _f32(x, "grad_sumsq input")
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    if workspace is None:
        workspace = grad_sumsq_workspace(x.numel(), x.device)
    if workspace.numel() * workspace.element_size() < L.lib().mi_grad_sumsq_workspace(x.numel()):
        raise ValueError("grad_sumsq: workspace too small")
    L.check(L.lib().mi_grad_sumsq(_p(x), x.numel(), _p(out), _p(workspace), _stream()), "grad_sumsq")
    return out


def adamw_step_ex(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, step: int, betas=(0.9, 0.999), eps: float = 1e-8,
                  weight_decay: float = 1e-2, grad_scale: float = 1.0, dev_scalars: Optional[Tensor] = None,
                  sumsq: Optional[Tensor] = None, max_norm: float = 0.0, norm_out: Optional[Tensor] = None,
                  ema: Optional[Tensor] = None, ema_decay: float = 0.0) -> None:
    """adamw_step with the gradient clipped by total norm (``sumsq``: device scalar sum of squares of ``g``, as grad_sumsq
    gives; the norm sqrt(sumsq) * grad_scale goes to ``norm_out``) and/or the EMA ``ema = ema*decay + p_new*(1-decay)``."""
    _gpu(p, g, m, v, dev_scalars, sumsq, norm_out, ema)
    for t in (p, g, m, v, ema):
        if t is not None and t.numel() != p.numel():
            raise ValueError("adamw_step_ex: p, g, m, v and ema must have the same number of elements")
    if sumsq is not None and not max_norm > 0:
        raise ValueError("adamw_step_ex: max_norm must be > 0")
    L.check(L.lib().mi_adamw_step_ex(_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), lr, betas[0], betas[1], eps, weight_decay,
                                     step, grad_scale, _p(dev_scalars), _p(sumsq), max_norm, _p(norm_out), ema_decay,
                                     _stream()), "adamw_step_ex")


def l1_loss(a: Tensor, b: Tensor, want_grad: bool = True, scale: float = 1.0):
    """mean|a-b| and (optionally) its gradient w.r.t. a times ``scale``; loss returned as a 1-element fp32 tensor."""
    _gpu(a, b)
    buf = torch.zeros(1 + 1024, dtype=torch.float32, device=a.device)
    da = torch.empty_like(a) if want_grad else None
    n = a.numel()
    L.check(L.lib().mi_l1_loss(_p(a), _p(b), _p(da), _p(buf), n, scale / n, _dt(a), _stream()), "l1_loss")
    return buf[:1], da


_FFT_L1_SECTIONS = ("cos_w", "sin_w", "cos_wt", "sin_wt", "cos_h", "sin_h", "T", "S", "partials", "reduce_scratch")


def fft_l1_plan(B: int, C: int, H: int, W: int, dtype: torch.dtype = torch.float32, want_grad: bool = True) -> dict:
    """What fft_l1_loss launches for [B, C, H, W] (mi_fft_l1_plan: the plan the launcher itself follows; no GPU work).
    ``sections`` maps each workspace section to its (byte offset, bytes); a grid of 0 means the stage is not launched."""
    out = (L.c_i64 * 40)()
    L.check(L.lib().mi_fft_l1_plan(B, C, H, W, _dtype_code(dtype), int(want_grad), out), "fft_l1_plan")
    keys = ("planes", "K", "tile_m", "tile_k", "l_block", "l_blocks", "x_block", "x_blocks", "m_tiles_folded", "m_tiles_plane",
            "grid_tables", "grid_stage1", "grid_stage2", "grid_stage3", "grid_stage4", "block", "partials", "reduce_launches",
            "launches")
    return _decode_report(out, keys, 19, _FFT_L1_SECTIONS, None, ("workspace",), 39)      # (its own report: out[40], one tail value)


def fft_l1_loss(pred: Tensor, target: Tensor, loss_weight: float = 1.0, want_grad: bool = True):
    """``loss_weight * mean(|Re| + |Im|)`` of ``rfft2(pred - target)`` over [B, C, H, W] and (optionally) its gradient w.r.t.
    pred in pred's dtype, as dense-DFT GEMMs on the fp32 MFMA (mi_fft_l1_loss: no FFT library, bitwise reproducible).  The
    loss comes back as a 1-element fp32 tensor.  2 <= H, W <= 512; anything else is an error."""
    _gpu(pred, target)
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"fft_l1_loss: pred and target must be [B, C, H, W] of one shape, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    if pred.dtype != target.dtype:
        raise TypeError(f"fft_l1_loss: pred and target must share a dtype, got {pred.dtype} and {target.dtype}")
    B, Cc, H, W = pred.shape
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = _ws(L.lib().mi_fft_l1_workspace(B, Cc, H, W), pred.device)
    L.check(L.lib().mi_fft_l1_loss(_p(pred), _p(target), _p(dpred), _p(loss), B, Cc, H, W, float(loss_weight), _dt(pred),
                                   _p(ws), _stream()), "fft_l1_loss")
    return loss, dpred


def _loss_pair(who: str, pred: Tensor, target: Tensor, planes: bool) -> None:
    _gpu(pred, target)
    if pred.shape != target.shape or (planes and pred.dim() != 4):
        raise ValueError(f"{who}: pred and target must be {'[B, C, H, W]' if planes else 'tensors'} of one shape, got "
                         f"{tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.dtype != target.dtype:
        raise TypeError(f"{who}: pred and target must share a dtype, got {pred.dtype} and {target.dtype}")


def ssim_loss(pred: Tensor, target: Tensor, loss_weight: float = 1.0, data_range: float = 1.0, want_grad: bool = True):
    """``pytorch_msssim.ssim`` with its defaults, restated (11-tap Gaussian, sigma 1.5, valid correlation, per channel; see
    include/mi_restore.h), over [B, C, H, W] with H, W >= 11.  Returns a 2-element fp32 tensor ``[loss_weight * (1 - m), m]``,
    m the mean SSIM, and (optionally) the gradient of its first entry w.r.t. pred in pred's dtype (mi_ssim_loss)."""
    _loss_pair("ssim_loss", pred, target, True)
    B, Cc, H, W = pred.shape
    if H < 11 or W < 11:
        raise ValueError(f"ssim_loss: H and W must be at least the 11-pixel window, got {H} x {W}")
    loss = torch.empty(2, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = _ws(L.lib().mi_ssim_loss_workspace(B, Cc, H, W), pred.device)
    L.check(L.lib().mi_ssim_loss(_p(pred), _p(target), _p(dpred), _p(loss), B, Cc, H, W, float(loss_weight), float(data_range),
                                 _dt(pred), _p(ws), _stream()), "ssim_loss")
    return loss, dpred


EDGE_CRITERIA = {"l2": 0, "l1": 1}


def edge_loss(pred: Tensor, target: Tensor, loss_weight: float = 1.0, criterion: str = "l2", want_grad: bool = True):
    """``loss_weight * mean(e^2)`` ('l2') or ``loss_weight * mean|e|`` ('l1') of e = Laplacian(pred - target), the Laplacian of
    the reference's EdgeLoss (5x5 blur over the replicate-padded plane, even-grid upsampling), over [B, C, H, W] with H, W >= 2,
    and (optionally) its gradient w.r.t. pred in pred's dtype (mi_edge_loss).  The loss is a 1-element fp32 tensor."""
    _loss_pair("edge_loss", pred, target, True)
    if criterion not in EDGE_CRITERIA:
        raise NotImplementedError(f"edge_loss: unsupported criterion {criterion!r} ('l1' or 'l2')")
    B, Cc, H, W = pred.shape
    if H < 2 or W < 2:
        raise ValueError(f"edge_loss: H and W must be at least 2, got {H} x {W}")
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = _ws(L.lib().mi_edge_loss_workspace(B, Cc, H, W), pred.device)
    L.check(L.lib().mi_edge_loss(_p(pred), _p(target), _p(dpred), _p(loss), B, Cc, H, W, float(loss_weight),
                                 EDGE_CRITERIA[criterion], _dt(pred), _p(ws), _stream()), "edge_loss")
    return loss, dpred


def focal_l1_loss(pred: Tensor, target: Tensor, gamma: float = 2.0, epsilon: float = 1e-6, alpha: float = 0.1,
                  scale: float = 1.0, want_grad: bool = True):
    """``scale * mean(log1p(a + epsilon)^gamma * a)``, a = |pred - target| / alpha (the reference's FocalL1Loss), over tensors of
    any shape, and (optionally) its gradient w.r.t. pred in pred's dtype, 0 at a tie (mi_focal_l1_loss).  1-element fp32 loss."""
    _loss_pair("focal_l1_loss", pred, target, False)
    if not alpha > 0:
        raise ValueError(f"focal_l1_loss: alpha must be > 0, got {alpha}")
    n = pred.numel()
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = _ws(L.lib().mi_focal_l1_workspace(n), pred.device)
    L.check(L.lib().mi_focal_l1_loss(_p(pred), _p(target), _p(dpred), _p(loss), n, float(gamma), float(epsilon), float(alpha),
                                     float(scale), _dt(pred), _p(ws), _stream()), "focal_l1_loss")
    return loss, dpred


# ----------------------------------------------------------------------------- profiler (bench.py roofline pass)
_pw_cache_buf: Optional[Tensor] = None


def pw_cache_enable(nbytes: int, device, params: Optional[Tensor] = None) -> Optional[Tensor]:
    """Lend the library a device buffer for packed 1x1 weights (include/mi_restore.h: mi_pw_cache_*).  `params` is the
    storage that holds the weights (e.g. the trainer's flat parameter buffer): only matrices inside it are cached.  The
    caller promises to call pw_cache_refresh() after every in-place weight update (or pw_cache_invalidate()).
    Returns the owner token (the lent buffer): hand it to pw_cache_release() - the cache is process-global, and only the
    object whose buffer it still points at may switch it off."""
    global _pw_cache_buf
    if nbytes <= 0 or params is None:
        L.check(L.lib().mi_pw_cache_enable(None, 0, None, None), "pw_cache_enable")
        _pw_cache_buf = None
        return None
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    lo = params.data_ptr()
    L.check(L.lib().mi_pw_cache_enable(buf.data_ptr(), nbytes, lo, lo + params.numel() * params.element_size()),
            "pw_cache_enable")
    _pw_cache_buf = buf  # keeps the memory alive for as long as the cache points at it
    return buf


def pw_cache_owner() -> Optional[Tensor]:
    return _pw_cache_buf


def pw_cache_release(token: Optional[Tensor]) -> bool:
    """Switch the cache off if (and only if) it still belongs to `token`'s owner.  A later owner (a second trainer, a
    PackedWeights made afterwards) keeps its cache when an earlier object is closed or garbage-collected."""
    global _pw_cache_buf
    if token is None or _pw_cache_buf is not token:
        return False
    L.check(L.lib().mi_pw_cache_enable(None, 0, None, None), "pw_cache_enable")
    _pw_cache_buf = None
    return True


def pw_cache_pending() -> bool:
    """True while the cache holds weights it has not packed yet (seen since the last refresh) or was invalidated."""
    return bool(L.lib().mi_pw_cache_pending())


def pw_cache_refresh() -> None:
    L.check(L.lib().mi_pw_cache_refresh(_stream()), "pw_cache_refresh")


def pw_cache_invalidate() -> None:
    L.check(L.lib().mi_pw_cache_invalidate(), "pw_cache_invalidate")


_deferred_arena: Optional[Tensor] = None


def deferred_begin(nbytes: int, device) -> Optional[Tensor]:
    """Lend the library an arena for deferred parameter-gradient reductions (include/mi_restore.h: mi_deferred_*): backward
    calls that accumulate into gradient buffers record their final sums instead of launching them; deferred_flush() runs them
    all in one launch.  Returns the owner token (the arena), or None when another owner already holds the context."""
    global _deferred_arena
    if _deferred_arena is not None:
        return None
    buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    L.check(L.lib().mi_deferred_begin(buf.data_ptr(), buf.numel()), "deferred_begin")
    _deferred_arena = buf
    return buf


def deferred_record(on: bool) -> None:
    """Producers defer only while recording is on: the owner brackets its backward window with it."""
    if _deferred_arena is not None:
        L.check(L.lib().mi_deferred_record(int(on)), "deferred_record")


def deferred_flush() -> None:
    if _deferred_arena is not None:
        L.check(L.lib().mi_deferred_flush(_stream()), "deferred_flush")


def deferred_pending() -> int:
    return int(L.lib().mi_deferred_pending()) if _deferred_arena is not None else 0


def deferred_end(token: Optional[Tensor]) -> bool:
    """Flush and close the deferral context if `token` owns it."""
    global _deferred_arena
    if token is None or _deferred_arena is not token:
        return False
    deferred_flush()
    deferred_record(False)
    L.check(L.lib().mi_deferred_end(), "deferred_end")
    _deferred_arena = None
    return True


def prof_enable(on: bool) -> None:
    L.check(L.lib().mi_prof_enable(int(on)), "prof_enable")


def prof_collect():
    """-> {kernel: dict(ms, bytes, flops, launches)} for kernels launched since prof_enable(True)."""
    lib = L.lib()
    n = lib.mi_prof_kernel_count()
    ms, by, fl = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    cnt = (L.c_i64 * n)()
    L.check(lib.mi_prof_collect(ms, by, fl, cnt, n), "prof_collect")
    out = {}
    for i in range(n):
        if cnt[i]:
            out[lib.mi_prof_kernel_name(i).decode()] = dict(ms=ms[i], bytes=by[i], flops=fl[i], launches=int(cnt[i]))
    return out


# ----------------------------------------------------------------------------- AdaIR frequency modules (csrc/adair.hip)
def box_down(img: Tensor, H: int, W: int) -> Tensor:
    """F.interpolate(img, (H, W), mode='bilinear') for the integer level factors (1, 2, 4, 8 ...)."""
    _gpu(img)
    B, Cc, Hi, Wi = img.shape
    if Hi % H or Wi % W or Hi // H != Wi // W:
        raise ValueError(f"box_down: {Hi}x{Wi} -> {H}x{W} is not an integer level factor")
    out = torch.empty((B, Cc, H, W), dtype=img.dtype, device=img.device)
    L.check(L.lib().mi_box_down(_p(img), _p(out), B, Cc, Hi, Wi, Hi // H, _dt(img), _stream()), "box_down")
    return out


def fre_rect(pooled: Tensor, w0: Tensor, w2: Tensor, H: int, W: int, n: int = 128) -> Tensor:
    _gpu(pooled, w0, w2)
    B, Cc = pooled.shape
    half = torch.empty((B, 2), dtype=torch.int32, device=pooled.device)
    L.check(L.lib().mi_fre_rect(_p(pooled), _p(w0), _p(w2), _p(half), B, Cc, w0.shape[0], H, W, n, _stream()), "fre_rect")
    return half


def fre_split_fwd(feat: Tensor, half: Optional[Tensor]):
    _gpu(feat, half)
    B, Cc, H, W = feat.shape
    high, low = torch.empty_like(feat), torch.empty_like(feat)
    coef = None
    if half is not None:
        coef = torch.empty(L.lib().mi_fre_split_coef_bytes(B, Cc) // 4, dtype=torch.float32, device=feat.device)
    L.check(L.lib().mi_fre_split_fwd(_p(feat), _p(half), _p(high), _p(low), _p(coef), B, Cc, H, W, _dt(feat), _stream()),
            "fre_split_fwd")
    return high, low, coef


def fre_split_bwd(feat: Tensor, half: Optional[Tensor], coef: Optional[Tensor], dhigh: Tensor, dlow: Tensor) -> Tensor:
    _gpu(feat, half, coef, dhigh, dlow)
    B, Cc, H, W = feat.shape
    dfeat = torch.empty_like(feat)
    ws = _ws(L.lib().mi_fre_split_workspace(B, Cc, H, W), feat.device)
    L.check(L.lib().mi_fre_split_bwd(_p(feat), _p(half), _p(coef), _p(dhigh), _p(dlow), _p(dfeat), B, Cc, H, W, _dt(feat),
                                     _p(ws), _stream()), "fre_split_bwd")
    return dfeat


def chan_maxmean_fwd(x: Tensor):
    _gpu(x)
    B, Cc, H, W = x.shape
    out = torch.empty((B, 2, H, W), dtype=x.dtype, device=x.device)
    idx = torch.empty((B, H * W), dtype=torch.int32, device=x.device)
    L.check(L.lib().mi_chan_maxmean_fwd(_p(x), _p(out), _p(idx), B, Cc, H * W, _dt(x), _stream()), "chan_maxmean_fwd")
    return out, idx


def chan_maxmean_bwd(dout: Tensor, idx: Tensor, Cc: int) -> Tensor:
    _gpu(dout, idx)
    B, _, H, W = dout.shape
    dx = torch.empty((B, Cc, H, W), dtype=dout.dtype, device=dout.device)
    L.check(L.lib().mi_chan_maxmean_bwd(_p(dout), _p(idx), _p(dx), B, Cc, H * W, _dt(dout), _stream()), "chan_maxmean_bwd")
    return dx


def plane_max_fwd(x: Tensor):
    _gpu(x)
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, Cc), dtype=torch.int32, device=x.device)
    L.check(L.lib().mi_plane_max_fwd(_p(x), _p(out), _p(idx), B * Cc, H * W, _dt(x), _stream()), "plane_max_fwd")
    return out, idx


def pool_pair_bwd(davg: Tensor, dmax: Tensor, idx: Tensor, like: Tensor) -> Tensor:
    _gpu(davg, dmax, idx)
    B, Cc, H, W = like.shape
    dx = torch.empty_like(like)
    L.check(L.lib().mi_pool_pair_bwd(_p(davg), _p(dmax), _p(idx), _p(dx), B * Cc, H * W, _dt(like), _stream()), "pool_pair_bwd")
    return dx


def chan_gate_fwd(avg: Tensor, mx: Tensor, w1: Tensor, w2: Tensor):
    _gpu(avg, mx, w1, w2)
    B, Cc = avg.shape
    R_ = w1.shape[0]
    cw = torch.empty_like(avg)
    hid = torch.empty((B, 2, R_), dtype=torch.float32, device=avg.device)
    L.check(L.lib().mi_chan_gate_fwd(_p(avg), _p(mx), _p(w1), _p(w2), _p(cw), _p(hid), B, Cc, R_, _stream()), "chan_gate_fwd")
    return cw, hid


def chan_gate_bwd(avg, mx, w1, w2, cw, hid, dcw, dw1, dw2, accumulate: bool):
    _gpu(avg, mx, w1, w2, cw, hid, dcw, dw1, dw2)
    B, Cc = avg.shape
    davg, dmx = torch.empty_like(avg), torch.empty_like(avg)
    L.check(L.lib().mi_chan_gate_bwd(_p(avg), _p(mx), _p(w1), _p(w2), _p(cw), _p(hid), _p(dcw), _p(davg), _p(dmx), _p(dw1), _p(dw2),
                                     B, Cc, w1.shape[0], int(accumulate), _stream()), "chan_gate_bwd")
    return davg, dmx


def refine_mix_fwd(low: Tensor, high: Tensor, s: Tensor, cw: Tensor) -> Tensor:
    _gpu(low, high, s, cw)
    B, Cc, H, W = low.shape
    out = torch.empty_like(low)
    L.check(L.lib().mi_refine_mix_fwd(_p(low), _p(high), _p(s), _p(cw), _p(out), B, Cc, H * W, _dt(low), _stream()), "refine_mix_fwd")
    return out


def refine_mix_bwd(low: Tensor, high: Tensor, s: Tensor, cw: Tensor, dout: Tensor):
    _gpu(low, high, s, cw, dout)
    B, Cc, H, W = low.shape
    dlow, dhigh, ds = torch.empty_like(low), torch.empty_like(low), torch.empty_like(s)
    dcw = torch.empty_like(cw)
    L.check(L.lib().mi_refine_mix_bwd(_p(low), _p(high), _p(s), _p(cw), _p(dout), _p(dlow), _p(dhigh), _p(ds), _p(dcw), B, Cc, H * W,
                                      _dt(low), _stream()), "refine_mix_bwd")
    return dlow, dhigh, ds, dcw


def scale_add_fwd(a: Tensor, y: Tensor, p1: Tensor, p2: Tensor) -> Tensor:
    _gpu(a, y, p1, p2)
    B, Cc, H, W = a.shape
    out = torch.empty_like(a)
    L.check(L.lib().mi_scale_add_fwd(_p(a), _p(y), _p(p1), _p(p2), _p(out), B, Cc, H * W, _dt(a), _stream()), "scale_add_fwd")
    return out


def scale_add_bwd(a: Tensor, y: Tensor, p1: Tensor, p2: Tensor, dout: Tensor, dp1: Tensor, dp2: Tensor, accumulate: bool):
    _gpu(a, y, p1, p2, dout, dp1, dp2)
    B, Cc, H, W = a.shape
    da, dy = torch.empty_like(a), torch.empty_like(a)
    L.check(L.lib().mi_scale_add_bwd(_p(a), _p(y), _p(p1), _p(p2), _p(dout), _p(da), _p(dy), _p(dp1), _p(dp2), B, Cc, H * W,
                                     int(accumulate), _dt(a), _stream()), "scale_add_bwd")
    return da, dy

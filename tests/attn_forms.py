"""Case tables, inputs, references, assertions and a CPU model of the attention c x c kernels and chan_sum (csrc/attn_small.hip).

Shared by tests/test_gpu_attn_small.py (which runs the kernels through ops.attn_small_fwd / attn_small_bwd / chan_sum) and
tests/test_cabi.py (which, without a GPU, checks that the tables reach every plan of the launchers, that the bounds admit correct
fp32 arithmetic in another summation order and that the assertions fail on five injected faults).  A plain module: no fixtures,
no pytest settings.

The entries need no pixel planes: graw = q k^T [Z,c,c] and ss = (|q_i|^2, |k_j|^2) [Z,2c] are all the fold reads of q and k, so a
case is a few MB.  Every row names the plan it must reach (instance CT, W_o row chunks per workgroup, chunks of the last row
group, raised-LDS launches); assert_plan() checks it against ops.attn_small_plan, so a threshold that moves in the launcher shows
up as a row that lost its plan.

Family A (exact): one-hot attention.  Norms are powers of two (ss = 4^k), graw[i][pi(i)] = nq_i nk_pi(i) for a permutation pi per
(image, head) and 0 elsewhere, temperature 200: P is exactly 1 or 0, expf(-200) is exactly 0, A is the permutation matrix, and
every index of the fold, of dW_o and of the bf16 / transposed copies is observable bit for bit (torch.equal).

Family B (float): random q, k over N = 2c + 8 pixels, graw and ss formed in fp64 and rounded to fp32.
  Reference 1: the formulas of the kernel header in fp64, from the rounded values (forward() / backward() below).
  Reference 2: fp64 autograd through F.normalize, softmax and the fold with the loss sum(M dM): independent of those formulas.
               reference_gap() holds Reference 1 to it (1e-10, every row, clamped rows included: it decides what a clamped norm
               means: x / max(|x|, eps) has NO projection term below eps, so D1 / D2 are 0 there and G1 is of order 1 / eps).
  Norms: each (image, head) block of P, A, M, dwo_part against its own maximum; wd after multiplying both sides by the reference
  norms (nq_i nk_j on the G1 blocks, nq_i^2 / nk_j^2 on the diagonals: every entry is then of the size of temperature dS), each
  block against its own maximum; dtemp_part[z] against sum |dS . P|, not against its own cancelled value; nrm per element.

MEASURED below is the error of evaluate_fp32() (torch fp32 on the CPU, natural order) against Reference 1 in those norms, the
largest over both tables (tools are not needed: measure() recomputes it).  The bound is 8 x that: the kernels sum in another order
(4-wide MFMA steps, 16-lane rows) and the device's expf and divisions are not the host's.  No bound exceeds the 5e-5 that the
block-level test (test_attention_small_kernels_at_padded_and_wide_heads) grants.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

EPS = float(np.float32(1e-12))               # NORM_EPS of the kernels, as the fp32 value they compare with
f32, f64, b16 = torch.float32, torch.float64, torch.bfloat16

# ---------------------------------------------------------------------------------------------- the two tables
# (B, C, heads) -> instance CT, promoted, rpw, chunks of the last row group, fold raised, backward raised
# Width table: c = C / heads over every instance at an exact and at a padded width and both promotions (ceil(c/16) = 5 -> CT 6,
# 7 -> CT 8).  C covers C % 16 != 0, C % 4 != 0 (scalar Mtb), C % 32 != 0 (the backward's 32-row staging tail), C % 64 != 0 with a
# last dW_o workgroup whose waves 1..3 hold no rows (C = 72), c % 4 != 0 (scalar wd).
WIDTH_CASES = (
    # B   C  heads   CT  promoted rpw last  fold^  bwd^        c
    ((2,   3, 3),   (1, False, 1, 1, False, False)),      #   1
    ((1,  30, 3),   (1, False, 1, 1, False, False)),      #  10
    ((3,  16, 1),   (1, False, 1, 1, False, False)),      #  16  exact
    ((2,  34, 2),   (2, False, 1, 1, False, False)),      #  17
    ((2,  72, 3),   (2, False, 1, 1, False, False)),      #  24  C = 72: the last dW_o workgroup has rows for wave 0 only
    ((2,  32, 1),   (2, False, 1, 1, False, False)),      #  32  exact
    ((1,  33, 1),   (3, False, 1, 1, False, False)),      #  33
    ((2,  80, 2),   (3, False, 1, 1, False, False)),      #  40
    ((3,  48, 1),   (3, False, 1, 1, False, False)),      #  48  exact
    ((2,  49, 1),   (4, False, 1, 1, False, False)),      #  49
    ((1, 128, 2),   (4, False, 1, 1, False, False)),      #  64  exact
    ((2,  65, 1),   (6, True,  1, 1, False, False)),      #  65  promoted, padded
    ((1,  80, 1),   (6, True,  1, 1, False, False)),      #  80  promoted
    ((1, 162, 2),   (6, False, 1, 1, False, False)),      #  81
    ((2,  96, 1),   (6, False, 1, 1, False, False)),      #  96  exact
    ((1,  97, 1),   (8, True,  1, 1, True,  True)),       #  97  promoted, padded
    ((2, 112, 1),   (8, True,  1, 1, True,  True)),       # 112  promoted
    ((1, 120, 1),   (8, False, 1, 1, True,  True)),       # 120
    ((1, 127, 1),   (8, False, 1, 1, True,  True)),       # 127
    ((1, 256, 2),   (8, False, 1, 1, True,  True)),       # 128  exact
)
# Chunk-plan table: what the fold does with several 16-row chunks of W_o per workgroup.
CHUNK_CASES = (
    ((8,    384, 8), (3, False, 2, 2, False, False)),     # rpw 2
    ((20,   384, 8), (3, False, 5, 4, False, False)),     # rpw 5, last group 4 of 24 chunks
    ((28,   384, 8), (3, False, 7, 3, False, False)),     # rpw 7, last group 3 chunks
    ((32,   384, 8), (3, False, 8, 8, False, False)),     # rpw 8: the benchmark's deepest level
    ((89,   200, 2), (8, True,  3, 1, True,  True)),      # CT 8, 13 chunks, rpw 3, last group 1 chunk, half-chunk row tail (200 = 12.5 x 16)
    ((160,  192, 2), (6, False, 5, 2, True,  False)),     # CT 6, rpw 5: the raised-LDS launch of that instance
    ((1536,  16, 1), (1, False, 1, 1, False, False)),     # 1536 / 768 = 2 asked for, capped at the single chunk
)
ALL_CASES = WIDTH_CASES + CHUNK_CASES
PLAN_KEYS = ("instance", "promoted", "rpw", "last_chunks", "fold_raised", "bwd_raised")
CLAMP_EVERY = 3                              # every third row of ALL_CASES gets clamped norms (is_clamp_case)

# chan_sum: (B, C, N) and, per dtype, (splits, pixels per split, vector path) for an aligned base
CHAN_SUM_CASES = (
    ((2,   3, 1000), {f32: (1, 1000, True),  b16: (1, 1000, True)}),       # one split
    ((2,  48, 4096), {f32: (4, 1024, True),  b16: (4, 1024, True)}),       # four splits
    ((3,   5, 5000), {f32: (5, 1000, True),  b16: (5, 1000, True)}),       # five splits of 1000
    ((1,   7, 5004), {f32: (5, 1008, True),  b16: (5, 1008, False)}),      # per split rounded up to 1008; 5004 % 8 = 4
    ((2,   4, 4099), {f32: (5,  824, False), b16: (5,  824, False)}),      # scalar path
    ((1, 600, 2048), {f32: (1, 2048, True),  b16: (1, 2048, True)}),       # more channels than 512: one split
)

# ---------------------------------------------------------------------------------------------- measured errors and bounds
# measure(ALL_CASES): error of evaluate_fp32 against Reference 1, largest over both tables, in the norms of the module docstring.
#   measured   nrm 6.32e-8   P 2.11e-7   A 3.37e-7   M 6.92e-7   dwo_part 7.88e-7   wd 1.125e-6   dtemp_part 6.52e-8
#   bound      nrm 5.12e-7   P 1.76e-6   A 2.72e-6   M 5.60e-6   dwo_part 6.32e-6   wd 9.04e-6    dtemp_part 5.28e-7   (8 x MEASURED, the figures above rounded up)
MEASURED = {"nrm": 6.4e-8, "P": 2.2e-7, "A": 3.4e-7, "M": 7.0e-7, "dwo_part": 7.9e-7, "wd": 1.13e-6, "dtemp_part": 6.6e-8}
FACTOR, CAP = 8.0, 5e-5
# Largest error of the kernels on an MI355X over both tables (printed per row by test_gpu_attn_small.py::test_attn_float): at the
# size of the host's own fp32 error, an eighth of the bound.
GPU_SEEN = {"nrm": 5.94e-8, "P": 2.10e-7, "A": 2.84e-7, "M": 6.26e-7, "dwo_part": 7.88e-7, "wd": 1.125e-6, "dtemp_part": 6.16e-8}
BOUND = {k: min(FACTOR * v, CAP) for k, v in MEASURED.items()}
REFERENCE_GAP = 1e-10                        # Reference 1 in fp64 on unrounded inputs against autograd


def case_id(case):
    (B, C, heads), _ = case
    return "B%d-C%d-h%d-c%d" % (B, C, heads, C // heads)


def is_clamp_case(case):
    return ALL_CASES.index(case) % CLAMP_EVERY == 0


def assert_plan(ops, case):
    """The plan of a row, after asserting that it is the one the row names."""
    (B, C, heads), want = case
    p = ops.attn_small_plan(B, C, heads)
    assert tuple(p[k] for k in PLAN_KEYS) == want, (case_id(case), {k: p[k] for k in PLAN_KEYS}, want)
    return p


def assert_chan_sum_plan(ops, B, C, N, dtype, aligned=True):
    want = dict(CHAN_SUM_CASES)[(B, C, N)][dtype]
    p = ops.chan_sum_plan(B, C, N, dtype, aligned)
    V = 16 // torch.empty(0, dtype=dtype).element_size()
    assert (p["splits"], p["per_split"]) == want[:2] and p["vector"] == (want[2] and aligned), (B, C, N, dtype, aligned, p)
    assert p["vector"] == (aligned and N % V == 0)
    return p


# ---------------------------------------------------------------------------------------------- inputs
def _gen(case, salt):
    (B, C, heads), _ = case
    return torch.Generator().manual_seed(1000003 * salt + 7919 * B + 31 * C + heads)


def clamp_rows(c, z):
    """(zeroed q row, zeroed k row, tiny q row, tiny k row) of block z: different rows in different blocks, the last row c - 1
    (inside the padded fragment whenever c % 16 != 0) among them; -1: none (c too small)."""
    zq = c - 1 if z % 2 == 0 else (5 * z + 2) % c
    zk = (zq + c // 2) % c if z % 2 == 0 else c - 1
    tq = (zq + 1) % c if c >= 4 else -1
    tk = (zk + 1) % c if c >= 4 else -1
    return zq, zk, tq, tk


def qk(case, clamp=None):
    """q, k [Z, c, N] in fp64, N = 2c + 8; row magnitudes spread over 2^-3 .. 2^3.  A clamp case has, per block, one all-zero q
    row and k row (norm 0, clamped to eps, a zero row / column of P) and one q row and k row of norm 2^-47 < eps (clamped, P not
    zero there: the only rows where a projection term that should be absent would show)."""
    (B, C, heads), _ = case
    clamp = is_clamp_case(case) if clamp is None else clamp
    c, Z = C // heads, B * heads
    N, g = 2 * c + 8, _gen(case, 1)
    q, k = torch.randn(Z, c, N, generator=g, dtype=f64), torch.randn(Z, c, N, generator=g, dtype=f64)
    q *= torch.exp2(torch.randint(-3, 4, (Z, c, 1), generator=g).double())
    k *= torch.exp2(torch.randint(-3, 4, (Z, c, 1), generator=g).double())
    if clamp:
        for z in range(Z):
            zq, zk, tq, tk = clamp_rows(c, z)
            if tq >= 0:
                q[z, tq] *= 2.0 ** -47 / q[z, tq].norm()
                k[z, tk] *= 2.0 ** -47 / k[z, tk].norm()
            q[z, zq] = 0
            k[z, zk] = 0
    return q, k


def _params(case, temperature=None):
    """temperature [heads], wo [C,C], dM [B,C,C] in fp32; dM's (image, head) column blocks are scaled by 2^-6 .. 2^6 so that a
    whole-tensor maximum would hide most of them."""
    (B, C, heads), _ = case
    c, g = C // heads, _gen(case, 2)
    temp = (torch.rand(heads, generator=g) * 3 + 0.5) if temperature is None else torch.full((heads,), float(temperature))
    wo = torch.randn(C, C, generator=g) / C ** 0.5
    dM = torch.randn(B, C, heads, c, generator=g) * torch.exp2(torch.randint(-6, 7, (B, 1, heads, 1), generator=g).float())
    return temp.float(), wo.float(), dM.reshape(B, C, C).float().contiguous()


def _case_ns(case, **kw):
    (B, C, heads), _ = case
    return types.SimpleNamespace(case=case, B=B, C=C, heads=heads, c=C // heads, Z=B * heads, **kw)


@functools.lru_cache(maxsize=2)
def float_inputs(case):
    """Family B: the fp32 tensors both the kernels and the references start from, and the fp64 Reference 1."""
    q, k = qk(case)
    graw = (q @ k.transpose(1, 2)).float()
    ss = torch.cat([(q * q).sum(-1), (k * k).sum(-1)], 1).float()
    temp, wo, dM = _params(case)
    s = _case_ns(case, graw=graw, ss=ss, temp=temp, wo=wo, dM=dM, clamp=is_clamp_case(case))
    s.ref = reference(s)
    # the backward starts from the forward's outputs as fp32 holds them: its error is then its own
    s.A, s.P, s.nrm = s.ref.A.float(), s.ref.P.float(), s.ref.nrm.float()
    s.ref_bwd = backward(s.dM.double(), s.A.double(), s.P.double(), s.nrm.double(), s.temp.double(), s.wo.double(), s.heads)
    return s


@functools.lru_cache(maxsize=2)
def exact_inputs(case):
    """Family A: one-hot attention (module docstring).  Everything the kernels must produce is known exactly."""
    (B, C, heads), _ = case
    c, Z, g = C // heads, B * heads, _gen(case, 3)
    nq, nk = torch.exp2(torch.randint(-3, 4, (Z, c), generator=g).float()), torch.exp2(torch.randint(-3, 4, (Z, c), generator=g).float())
    perm = torch.stack([torch.randperm(c, generator=g) for _ in range(Z)])               # pi(i)
    onehot = torch.zeros(Z, c, c).scatter_(2, perm[:, :, None], 1.0)
    graw = onehot * nq[:, :, None] * nk[:, None, :]
    temp, wo, dM = _params(case, temperature=200.0)
    s = _case_ns(case, graw=graw, ss=torch.cat([nq * nq, nk * nk], 1), temp=temp, wo=wo, dM=dM, clamp=False, perm=perm)
    s.nrm, s.P, s.A = torch.cat([nq, nk], 1), onehot, onehot
    inv = torch.argsort(perm, 1)                                                         # pi^-1(j)
    cols = (torch.arange(heads)[None, :, None] * c + inv.view(B, heads, c)).reshape(B, C)  # M[b][:, hc+j] = wo[:, hc+pi^-1(j)]
    s.M = torch.stack([wo[:, cols[b]] for b in range(B)])
    colp = (torch.arange(heads)[None, :, None] * c + perm.view(B, heads, c)).reshape(B, C)  # dwo_part[b][:, hc+i] = dM[b][:, hc+pi(i)]
    s.dwo_part = torch.stack([dM[b][:, colp[b]] for b in range(B)])
    return s


# ---------------------------------------------------------------------------------------------- Reference 1: the header's formulas
def forward(graw, ss, temp, wo, heads, eps=EPS):
    """nrm, P, S-softmax A and the fold M, in the dtype of the arguments."""
    Z, c, _ = graw.shape
    B, C = Z // heads, wo.shape[0]
    nrm = ss.sqrt().clamp_min(eps)
    nq, nk = nrm[:, :c], nrm[:, c:]
    P = graw / (nq[:, :, None] * nk[:, None, :])
    A = torch.softmax(P * temp.repeat(B)[:, None, None], -1)
    M = torch.einsum("rhi,bhij->brhj", wo.view(C, heads, c), A.view(B, heads, c, c)).reshape(B, C, C)
    return types.SimpleNamespace(nrm=nrm, P=P, A=A, M=M)


def backward(dM, A, P, nrm, temp, wo, heads, eps=EPS, d_on_clamp=False):
    """dwo_part, dtemp_part, wd = [[G1, diag D1], [diag D2, G1^T]] and what the norms of the comparison need (dsp = sum |dS . P|,
    scale = the reference norms per entry of wd)."""
    Z, c, _ = A.shape
    B, C = Z // heads, wo.shape[0]
    nq, nk = nrm[:, :c], nrm[:, c:]
    t = temp.repeat(B)[:, None, None]
    Wh, dMh = wo.view(C, heads, c), dM.view(B, C, heads, c)
    dA = torch.einsum("rhi,brhj->bhij", Wh, dMh).reshape(Z, c, c)
    dwo = torch.einsum("brhj,bhij->brhi", dMh, A.view(B, heads, c, c)).reshape(B, C, C)
    dS = A * (dA - (dA * A).sum(-1, keepdim=True))
    sp = dS * P
    G1 = t * dS / (nq[:, :, None] * nk[:, None, :])
    D1 = -(t * sp).sum(2) / nq ** 2
    D2 = -(t * sp).sum(1) / nk ** 2
    if not d_on_clamp:                       # x / max(|x|, eps): no projection term where the norm was clamped
        D1, D2 = D1 * (nq > eps), D2 * (nk > eps)
    wd = torch.zeros(Z, 2 * c, 2 * c, dtype=A.dtype)
    wd[:, :c, :c], wd[:, c:, c:] = G1, G1.transpose(1, 2)
    wd[:, :c, c:], wd[:, c:, :c] = torch.diag_embed(D1), torch.diag_embed(D2)
    scale = torch.zeros_like(wd)
    scale[:, :c, :c] = nq[:, :, None] * nk[:, None, :]
    scale[:, c:, c:] = scale[:, :c, :c].transpose(1, 2)
    scale[:, :c, c:], scale[:, c:, :c] = torch.diag_embed(nq ** 2), torch.diag_embed(nk ** 2)
    return types.SimpleNamespace(dwo_part=dwo, dtemp_part=sp.sum((1, 2)), wd=wd, dsp=sp.abs().sum((1, 2)), scale=scale)


def reference(s):
    return forward(s.graw.double(), s.ss.double(), s.temp.double(), s.wo.double(), s.heads)


# ---------------------------------------------------------------------------------------------- Reference 2: autograd
def reference_gap(case, d_on_clamp=False):
    """Reference 1, evaluated in fp64 on the UNROUNDED q, k of a row, against fp64 autograd through F.normalize, softmax and the
    fold with the loss sum(M dM): the largest of the errors of M, of wd applied to the stacked [k; q] against dq / dk, of dwo_part
    summed over images against dW_o and of dtemp_part summed against d temperature, each relative to the block's / tensor's
    maximum.  (dq, dk rows are compared row by row: a clamped row's gradient is 1e12 times its neighbours'.)  d_on_clamp: with
    the projection terms D1 / D2 kept on clamped norms, which autograd rejects on the rows of norm 2^-47."""
    (B, C, heads), _ = case
    c, Z = C // heads, B * heads
    q, k = qk(case)
    temp, wo, dM = (t.double() for t in _params(case))
    qa, ka, ta, wa = (t.clone().requires_grad_(True) for t in (q, k, temp, wo))
    qn, kn = F.normalize(qa, dim=-1, eps=EPS), F.normalize(ka, dim=-1, eps=EPS)
    A = torch.softmax((qn @ kn.transpose(1, 2)).view(B, heads, c, c) * ta[None, :, None, None], -1)
    M = torch.einsum("rhi,bhij->brhj", wa.view(C, heads, c), A).reshape(B, C, C)
    (M * dM).sum().backward()
    r = forward(q @ k.transpose(1, 2), torch.cat([(q * q).sum(-1), (k * k).sum(-1)], 1), temp, wo, heads)
    g = backward(dM, r.A, r.P, r.nrm, temp, wo, heads, d_on_clamp=d_on_clamp)
    act = g.wd @ torch.cat([k, q], 1)

    def rows(a, b):
        return float(((a - b).abs().amax(-1) / b.abs().amax(-1).clamp_min(1e-300)).max())
    gaps = {"M": rows(r.M.reshape(B, -1), M.detach().reshape(B, -1)), "dq": rows(act[:, :c], qa.grad), "dk": rows(act[:, c:], ka.grad),
            "dwo": rows(g.dwo_part.sum(0).reshape(1, -1), wa.grad.reshape(1, -1)),
            "dtemp": float(((g.dtemp_part.view(B, heads).sum(0) - ta.grad).abs() / g.dsp.view(B, heads).sum(0).clamp_min(1e-300)).max())}
    return gaps


# ---------------------------------------------------------------------------------------------- the fp32 model on the CPU
FAULTS = ("pad_in_softmax", "partial_group_unwritten", "d_on_clamp", "g1t_shift", "mtb_tail")


def evaluate_fp32(s, plan, seed=None, fault=None):
    """The two kernels in torch fp32 on the CPU: every output they write, bf16 copies included, from the inputs of a case.
    seed: permute every contraction (the i of the fold, the rows r of dA, the j of dW_o and of the row sums) - the same sums in
    another order.  fault: one of FAULTS, the kind of mistake the kernels' padding, row groups, clamps and vector tails can make."""
    B, C, heads, c, Z = s.B, s.C, s.heads, s.c, s.Z
    g = torch.Generator().manual_seed(seed) if seed is not None else None

    def perm(n):
        return torch.randperm(n, generator=g) if g is not None else torch.arange(n)
    # ---- forward
    nrm = s.ss.sqrt().clamp_min(EPS)
    nq, nk = nrm[:, :c], nrm[:, c:]
    P = s.graw * (1.0 / nq)[:, :, None] * (1.0 / nk)[:, None, :]
    S = P * s.temp.repeat(B)[:, None, None]
    e = torch.exp(S - S.amax(-1, keepdim=True))
    pj = perm(c)
    den = e[:, :, pj].sum(-1, keepdim=True)
    if fault == "pad_in_softmax":            # the padding columns j >= c of the 16 CT wide tile take part with score 0
        den = den + (plan["padded"] - c) * torch.exp(-S.amax(-1, keepdim=True))
    A = e / den
    pi = perm(c)
    M = torch.einsum("rhi,bhij->brhj", s.wo.view(C, heads, c)[:, :, pi], A.view(B, heads, c, c)[:, :, pi]).reshape(B, C, C).contiguous()
    if fault == "partial_group_unwritten":   # the last row group holds fewer chunks than rpw: its last chunk's rows never stored
        assert plan["last_chunks"] < plan["rpw"]
        M[:, 16 * ((C + 15) // 16 - 1):] = float("nan")
    Mb = M.to(b16)
    Mtb = Mb.transpose(1, 2).contiguous()
    if fault == "mtb_tail" and C % 4:        # the scalar tail of the transposed store writes [r][j] where [j][r] belongs
        Mtb[:, :, C - C % 4:] = Mb[:, :, C - C % 4:]
    out = {"nrm": nrm, "P": P, "A": A, "M": M, "Mb": Mb, "Mtb": Mtb}
    # ---- backward, from the case's A, P, nrm (the references' values in fp32), as the kernel is given them
    A, P, nq, nk = s.A, s.P, s.nrm[:, :c], s.nrm[:, c:]
    t = s.temp.repeat(B)[:, None, None]
    Wh, dMh = s.wo.view(C, heads, c), s.dM.view(B, C, heads, c)
    pr = perm(C)
    dA = torch.einsum("rhi,brhj->bhij", Wh[pr], dMh[:, pr]).reshape(Z, c, c)
    dwo = torch.einsum("brhj,bhij->brhi", dMh[..., pj], A.view(B, heads, c, c)[..., pj]).reshape(B, C, C)
    dS = A * (dA - (dA * A)[:, :, pj].sum(-1, keepdim=True))
    sp = dS * P
    G1 = t * dS / (nq[:, :, None] * nk[:, None, :])
    D1, D2 = -(t * sp)[:, :, pj].sum(2) / (nq * nq), -(t * sp)[:, pi, :].sum(1) / (nk * nk)
    if fault != "d_on_clamp":
        D1, D2 = D1 * (nq > EPS), D2 * (nk > EPS)
    wd = torch.zeros(Z, 2 * c, 2 * c)
    wd[:, :c, :c], wd[:, c:, c:] = G1, G1.transpose(1, 2)
    wd[:, :c, c:], wd[:, c:, :c] = torch.diag_embed(D1), torch.diag_embed(D2)
    if fault == "g1t_shift" and c % 4:       # the scalar tail of the transposed G1 store is off by one row of G1
        i0 = c - c % 4
        wd[:, c:, c + i0:] = G1[:, i0 - 1:c - 1].transpose(1, 2) if i0 else G1.roll(1, 1).transpose(1, 2)
    out.update(dwo_part=dwo, dtemp_part=sp[:, :, pj].sum(2)[:, pi].sum(1), wd=wd, wdb=wd.to(b16))
    return out


# ---------------------------------------------------------------------------------------------- norms and assertions
def _blocks_zcc(x, s):
    return x.reshape(s.Z, -1)


def _blocks_bcc(x, s):                       # [B,C,C] -> [Z, C*c]: the column block of each head
    return x.reshape(s.B, s.C, s.heads, s.c).permute(0, 2, 1, 3).reshape(s.Z, -1)


def block_error(got, ref, blocks, s):
    """max over (image, head) blocks of max|got - ref| / max|ref| within the block."""
    g, r = blocks(got.double(), s), blocks(ref, s)
    return float(((g - r).abs().amax(1) / r.abs().amax(1).clamp_min(1e-300)).max())


def errors_fwd(got, s):
    r = s.ref
    return {"nrm": float(((got["nrm"].double() - r.nrm).abs() / r.nrm).max()), "P": block_error(got["P"], r.P, _blocks_zcc, s),
            "A": block_error(got["A"], r.A, _blocks_zcc, s), "M": block_error(got["M"], r.M, _blocks_bcc, s)}


def errors_bwd(got, s):
    r = s.ref_bwd
    return {"dwo_part": block_error(got["dwo_part"], r.dwo_part, _blocks_bcc, s),
            "wd": block_error(got["wd"].double() * r.scale, r.wd * r.scale, _blocks_zcc, s),
            "dtemp_part": float(((got["dtemp_part"].double() - r.dtemp_part).abs() / r.dsp.clamp_min(1e-300)).max())}


def assert_written(got, names, who):
    for n in names:
        if got.get(n) is not None:
            assert not torch.isnan(got[n].float()).any(), f"{who}: {n} has elements never written (or NaN)"


def assert_copies_fwd(got, who):
    """Mb is M rounded to bf16 and Mtb its transpose per image, bit for bit (either may be absent)."""
    if got.get("Mb") is not None:
        assert torch.equal(got["Mb"], got["M"].to(b16)), f"{who}: Mb is not M in bf16"
    if got.get("Mtb") is not None:
        assert torch.equal(got["Mtb"], got["M"].to(b16).transpose(1, 2)), f"{who}: Mtb is not Mb transposed"


def assert_structure_bwd(got, s, who):
    """What holds exactly whatever the data: zero off-diagonals of the D1 / D2 blocks, the lower-right block the upper-left one
    transposed, wdb the bf16 rounding of wd; D1 / D2 zero where the norm was clamped."""
    c, wd = s.c, got["wd"]
    off = ~torch.eye(c, dtype=torch.bool)
    assert (wd[:, :c, c:][:, off] == 0).all() and (wd[:, c:, :c][:, off] == 0).all(), f"{who}: off-diagonal of D1 / D2 not zero"
    assert torch.equal(wd[:, c:, c:], wd[:, :c, :c].transpose(1, 2)), f"{who}: lower-right block is not G1 transposed"
    if got.get("wdb") is not None:
        assert torch.equal(got["wdb"], wd.to(b16)), f"{who}: wdb is not wd in bf16"
    d1, d2 = torch.diagonal(wd[:, :c, c:], dim1=1, dim2=2), torch.diagonal(wd[:, c:, :c], dim1=1, dim2=2)
    clq, clk = s.nrm[:, :c] <= EPS, s.nrm[:, c:] <= EPS
    assert (d1[clq] == 0).all() and (d2[clk] == 0).all(), f"{who}: D1 / D2 not zero on a clamped norm"
    return int(clq.sum() + clk.sum())


def assert_float_fwd(got, s, who):
    """Family B, forward.  Returns error / bound per output."""
    assert_written(got, ("nrm", "P", "A", "M", "Mb", "Mtb"), who)
    assert all(torch.isfinite(got[n]).all() for n in ("nrm", "P", "A", "M")), f"{who}: not finite"
    assert_copies_fwd(got, who)
    if s.clamp:
        c = s.c
        for z in range(s.Z):
            zq, zk, tq, tk = clamp_rows(c, z)
            for row, base in ((zq, 0), (tq, 0), (zk, c), (tk, c)):
                assert row < 0 or float(got["nrm"][z, base + row]) == EPS, f"{who}: nrm not clamped at block {z} row {row}"
            assert (got["P"][z, zq] == 0).all() and (got["P"][z, :, zk] == 0).all(), f"{who}: P not zero on a zero row at block {z}"
    e = errors_fwd(got, s)
    for n, v in e.items():
        assert v <= BOUND[n], f"{who}: {n} off, {v:.3e} > {BOUND[n]:.3e}"
    return {n: v / BOUND[n] for n, v in e.items()}, e


def assert_float_bwd(got, s, who):
    """Family B, backward.  Returns error / bound per output."""
    assert_written(got, ("dwo_part", "dtemp_part", "wd", "wdb"), who)
    assert all(torch.isfinite(got[n]).all() for n in ("dwo_part", "dtemp_part", "wd")), f"{who}: not finite"
    clamped = assert_structure_bwd(got, s, who)
    assert (clamped > 0) == s.clamp
    e = errors_bwd(got, s)
    for n, v in e.items():
        assert v <= BOUND[n], f"{who}: {n} off, {v:.3e} > {BOUND[n]:.3e}"
    return {n: v / BOUND[n] for n, v in e.items()}, e


def assert_exact_fwd(got, s, who):
    """Family A, forward: every output bit for bit."""
    assert_written(got, ("nrm", "P", "A", "M", "Mb", "Mtb"), who)
    for n in ("nrm", "P", "A", "M"):
        assert torch.equal(got[n], getattr(s, n)), f"{who}: {n} differs"
    assert_copies_fwd(got, who)


def assert_exact_bwd(got, s, who):
    """Family A, backward on the one-hot A: dwo_part is a column permutation of dM, dS is exactly zero."""
    assert_written(got, ("dwo_part", "dtemp_part", "wd", "wdb"), who)
    assert torch.equal(got["dwo_part"], s.dwo_part), f"{who}: dwo_part differs"
    for n in ("wd", "wdb", "dtemp_part"):
        assert got.get(n) is None or (got[n] == 0).all(), f"{who}: {n} not zero"


def measure(cases=ALL_CASES):
    """MEASURED, recomputed: the largest error of the natural-order fp32 evaluation over `cases`, per output."""
    worst = {}
    for case in cases:
        s = float_inputs(case)
        got = evaluate_fp32(s, {"padded": 0, "rpw": 1, "last_chunks": 1})
        for n, v in {**errors_fwd(got, s), **errors_bwd(got, s)}.items():
            worst[n] = max(worst.get(n, 0.0), v)
    return worst


# ---------------------------------------------------------------------------------------------- running the kernels (GPU)
BAND, SENTINEL = 64, -7.0                    # 64 elements: the outputs keep the 16-byte alignment the vector stores rely on


class Guarded:
    """Output buffers prefilled with NaN between two bands of SENTINEL."""
    def __init__(self, device):
        self.device, self.flat = device, {}

    def new(self, name, shape, dtype):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * BAND,), float("nan"), dtype=dtype, device=self.device)
        buf[:BAND] = SENTINEL
        buf[BAND + n:] = SENTINEL
        self.flat[name] = (buf, n)
        return buf[BAND:BAND + n].view(shape)

    def check(self, who):
        for name, (buf, n) in self.flat.items():
            assert (buf[:BAND] == SENTINEL).all() and (buf[BAND + n:] == SENTINEL).all(), f"{who}: wrote outside {name}"


def run_fwd(ops, s, device, mb=True, mtb=True, who=""):
    g = Guarded(device)
    Z, c, B, C = s.Z, s.c, s.B, s.C
    out = {"P": g.new("P", (Z, c, c), f32), "A": g.new("A", (Z, c, c), f32), "nrm": g.new("nrm", (Z, 2 * c), f32),
           "M": g.new("M", (B, C, C), f32)}
    if mb:
        out["Mb"] = g.new("Mb", (B, C, C), b16)
    if mtb:
        out["Mtb"] = g.new("Mtb", (B, C, C), b16)
    got = ops.attn_small_fwd(s.graw.to(device), s.ss.to(device), s.temp.to(device), s.wo.to(device), s.heads, out=out)
    g.check(who)
    return {k: (v.cpu() if v is not None else None) for k, v in got.items()}


def run_bwd(ops, s, device, wdb=True, who=""):
    g = Guarded(device)
    Z, c, B, C = s.Z, s.c, s.B, s.C
    out = {"dwo_part": g.new("dwo_part", (B, C, C), f32), "dtemp_part": g.new("dtemp_part", (Z,), f32),
           "wd": g.new("wd", (Z, 2 * c, 2 * c), f32)}
    if wdb:
        out["wdb"] = g.new("wdb", (Z, 2 * c, 2 * c), b16)
    got = ops.attn_small_bwd(s.dM.to(device), s.A.to(device), s.P.to(device), s.nrm.to(device), s.temp.to(device), s.wo.to(device),
                             s.heads, out=out)
    g.check(who)
    return {k: (v.cpu() if v is not None else None) for k, v in got.items()}

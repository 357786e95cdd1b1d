"""The attention c x c kernels (attn_fold_kernel, attn_bwd_kernel) and chan_sum (csrc/attn_small.hip) on their own, at every
instance width, chunk plan and clamp.

The tables, inputs, references, bounds and assertions live in tests/attn_forms.py; tests/test_cabi.py checks without a GPU that the
tables reach every plan, that the bounds admit correct fp32 arithmetic and that the assertions fail on five injected faults.
Every case first asserts from ops.attn_small_plan / ops.chan_sum_plan that the call reaches the plan its row names, then runs the
kernel through ops.attn_small_fwd / attn_small_bwd / chan_sum on NaN-prefilled outputs between sentinel bands.

Family A (one-hot attention) is compared bit for bit.  Family B (random data, clamped norms on every third row) is held, per
(image, head) block, to 8 x the error of a torch fp32 evaluation on the CPU (attn_forms.MEASURED / BOUND).  Largest error of the
kernels on an MI355X over both tables, as printed by test_attn_float (attn_forms.GPU_SEEN), against the bound:
    nrm 5.94e-8 / 5.12e-7   P 2.10e-7 / 1.76e-6   A 2.84e-7 / 2.72e-6   M 6.26e-7 / 5.60e-6   dwo_part 7.88e-7 / 6.32e-6
    wd 1.125e-6 / 9.04e-6   dtemp_part 6.16e-8 / 5.28e-7"""
import pytest
import torch

import attn_forms as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
_cases = pytest.mark.parametrize("case", T.ALL_CASES, ids=T.case_id)


def ops():
    from image_restoration_amd import ops as o
    return o


@_cases
def test_attn_exact(case):
    """Family A: nrm, P, A, the fold M with its bf16 copy and transposed copy, and dwo_part bit for bit; wd, wdb, dtemp_part
    exactly zero."""
    o, who = ops(), T.case_id(case)
    T.assert_plan(o, case)
    s = T.exact_inputs(case)
    T.assert_exact_fwd(T.run_fwd(o, s, DEV, who=who), s, who)
    T.assert_exact_bwd(T.run_bwd(o, s, DEV, who=who), s, who)


@_cases
def test_attn_float(case):
    """Family B: every output within its bound of the fp64 Reference 1 in the per-block norms, the exact structure of wd, the bf16
    copies, and on the clamp rows nrm = eps, zero rows / columns of P and D1 = D2 = 0."""
    o, who = ops(), T.case_id(case)
    T.assert_plan(o, case)
    s = T.float_inputs(case)
    fwd, bwd = T.run_fwd(o, s, DEV, who=who), T.run_bwd(o, s, DEV, who=who)
    print("\n%s clamp=%d errors: %s" % (who, s.clamp, " ".join("%s %.3e" % kv for kv in {**T.errors_fwd(fwd, s), **T.errors_bwd(bwd, s)}.items())))
    T.assert_float_fwd(fwd, s, who)
    T.assert_float_bwd(bwd, s, who)


@pytest.mark.parametrize("case", [T.WIDTH_CASES[3], T.WIDTH_CASES[4], T.WIDTH_CASES[15], T.CHUNK_CASES[1], T.CHUNK_CASES[4]], ids=T.case_id)
def test_attn_optional_copies_and_repeat(case):
    """Without Mb / Mtb (as the fused MDTA path calls the fold) and without wdb the fp32 outputs keep their bits, and a second call
    gives the same bits as the first."""
    o, who = ops(), T.case_id(case)
    T.assert_plan(o, case)
    s = T.float_inputs(case)
    fwd, bwd = T.run_fwd(o, s, DEV, who=who), T.run_bwd(o, s, DEV, who=who)
    again_f, again_b = T.run_fwd(o, s, DEV, who=who), T.run_bwd(o, s, DEV, who=who)
    assert all(torch.equal(fwd[k], again_f[k]) for k in fwd) and all(torch.equal(bwd[k], again_b[k]) for k in bwd), who
    for mb, mtb in ((True, False), (False, True), (False, False)):
        bare = T.run_fwd(o, s, DEV, mb=mb, mtb=mtb, who=who)
        assert (bare["Mb"] is not None) == mb and (bare["Mtb"] is not None) == mtb
        assert all(torch.equal(fwd[k], bare[k]) for k in fwd if bare[k] is not None), (who, mb, mtb)
    bare = T.run_bwd(o, s, DEV, wdb=False, who=who)
    assert bare["wdb"] is None and all(torch.equal(bwd[k], bare[k]) for k in ("dwo_part", "dtemp_part", "wd")), who


def _ints(B, C, N, dtype, seed, offset=0):
    """Integers in [-8, 8] as [B, C, 1, N] on the device, `offset` elements off the allocation's (16-byte aligned) base."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (B, C, 1, N), generator=g).to(dtype)
    buf = torch.empty(x.numel() + 8, dtype=dtype, device=DEV)
    view = buf[offset:offset + x.numel()].view(B, C, 1, N)
    view.copy_(x)
    assert (view.data_ptr() % 16 == 0) == (offset == 0) and view.is_contiguous()
    return view, x.double().sum((0, 2, 3)).float()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [k for k, _ in T.CHAN_SUM_CASES], ids=lambda s: "B%d-C%d-N%d" % s)
def test_chan_sum_exact(shape, dtype):
    """chan_sum on small integers equals the host sum bit for bit: one split and several, per-split bounds rounded to 8, the vector
    and the scalar path, a base one element off the 16-byte grid, and accumulation onto a prior value."""
    o = ops()
    B, C, N = shape
    for offset in (0, 1):
        p = T.assert_chan_sum_plan(o, B, C, N, dtype, aligned=offset == 0)
        assert offset == 0 or not p["vector"]
        x, ref = _ints(B, C, N, dtype, 17 * C + N, offset)
        out = o.chan_sum(x)
        assert torch.equal(out.cpu(), ref), (shape, dtype, offset, float((out.cpu() - ref).abs().max()))
        prior = torch.arange(C, dtype=torch.float32) - 3
        acc = prior.to(DEV)
        assert o.chan_sum(x, acc, True) is acc and torch.equal(acc.cpu(), prior + ref), (shape, dtype, offset)
        assert torch.equal(o.chan_sum(x).cpu(), ref)                      # and again: the same bits


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_chan_sum_deferred_equals_immediate(dtype):
    """The accumulating call inside ops.deferred_begin .. flush leaves the gradient untouched until the flush and then holds the
    immediate call's bits."""
    o = ops()
    token = o.deferred_begin(8 << 20, torch.device(DEV))
    assert token is not None, "another owner holds the deferral context"
    try:
        o.deferred_record(True)
        for B, C, N in ((3, 5, 5000), (1, 7, 5004), (2, 3, 1000)):
            T.assert_chan_sum_plan(o, B, C, N, dtype)
            x, ref = _ints(B, C, N, dtype, 5 * C + N)
            prior = torch.arange(C, dtype=torch.float32) + 2
            o.deferred_record(False)
            now = o.chan_sum(x, prior.to(DEV), True)
            o.deferred_record(True)
            later = prior.to(DEV)
            o.chan_sum(x, later, True)
            assert o.deferred_pending() == 1 and torch.equal(later.cpu(), prior)
            o.deferred_flush()
            assert o.deferred_pending() == 0 and torch.equal(later, now) and torch.equal(now.cpu(), prior + ref), (B, C, N, dtype)
    finally:
        assert o.deferred_end(token)

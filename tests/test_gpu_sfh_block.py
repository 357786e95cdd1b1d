"""SFHformer's Block and Stage on the MI355X.  The node is a launch sequence over entry points that are tested where they live, so
its correctness rests on exact comparisons: against the same sequence written here with the ops of the parts (1), against the
public modules chained under autograd (2), then the reference fixtures (3), main_grad accumulation (4), poisoned buffers and
repeated runs (5), no_grad and eval mode (6), and the refusals (7).  The cases are tests/sfh_block_ref.py's: an odd plane (the
narrow access form), segment width 3, dim 32, two chunks per plane (the seam merges pairs), Stages of depth 2 and 3."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import sfh_block_ref as R  # noqa: E402
import sfh_ffn_ref as FR  # noqa: E402
import sfh_mixer_ref as M  # noqa: E402
from oracle.fixtures import check, load, seeded_input  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
MODES = pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
BLOCK_CASES = [n for n, c in R.CASES.items() if c[0] in ("block", "stage")]


def N():
    from image_restoration_amd import sfhformer
    return sfhformer


def O():
    from image_restoration_amd import ops
    return ops


def build(kind, args, sd, training=True):
    n = N()
    mod = {"block": n.Block, "stage": n.Stage, "net": n.Backbone}[kind](**args)
    mod.load_state_dict(R.module_state(kind, args, sd), strict=True)
    return mod.to(DEV).train(training)


def run_native(mod, kind, args, x, cot, dtype, forward=None):
    """Forward (``forward(mod, x)``, else the module itself) and backward -> {name: CPU tensor} over R.tensors(kind, args)."""
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    y = forward(mod, xg) if forward else mod(xg)
    y.backward(cot.to(DEV).to(dtype))
    torch.cuda.synchronize()
    sd = mod.state_dict()
    out = {"y": y.detach().cpu(), "dx": xg.grad.detach().cpu()}
    out.update({"g." + k: p.grad.detach().cpu() for k, p in mod.named_parameters()})
    out.update({"buf." + k: sd[k].cpu().clone() for k in R.buffers_of(kind, args)})
    return out


def counters(mod):
    return [int(v) for k, v in mod.state_dict().items() if k.endswith("num_batches_tracked")]


# ------------------------------------------------------------------ the public modules chained under autograd
def chain_block(blk, x):
    n = N()
    x1 = n.scaled_residual(blk.mixer(blk.norm1(x)), x, blk.beta)
    return n.scaled_residual(blk.ffn(blk.norm2(x1)), x1, blk.gamma)


def chain_stage(stage, x):
    for blk in stage.blocks:
        x = chain_block(blk, x)
    return x


def chain(mod, x):
    return chain_block(mod, x) if isinstance(mod, N().Block) else chain_stage(mod, x)


# ------------------------------------------------------------------ the op sequence of the issue, written with the parts' ops
def op_sequence(kind, args, sd, x, cot, dtype, training):
    """BatchNorm (part_in) -> Mixer -> scaled residual (want_part) -> BatchNorm (part_in) -> FFN -> scaled residual, block by block,
    and the backward with dres; every call through ops.bn2d_* / sfh_mixer_* / sfh_ffn_* / scale_res_*.  -> R.tensors(kind, args)."""
    ops = O()
    P = {k: v.to(DEV).clone() for k, v in sd.items()}
    G = {k: torch.full_like(P[k], float("nan")) for k in R.params_of(kind, args)}
    prefixes = R.block_prefixes(kind, args)
    xd, part, ctxs = x.to(DEV).to(dtype), None, []
    for i, pre in enumerate(prefixes):
        stats = [P[f"{pre}{n}.running_{s}"] for n in R.BLOCK_NORMS for s in ("mean", "var")]
        mp, fp = [P[pre + "mixer." + k] for k in M.MIXER_PARAMS], [P[pre + "ffn." + k] for k in FR.FFN_PARAMS]
        y1, st1 = ops.bn2d_fwd(xd, P[pre + "norm1.weight"], P[pre + "norm1.bias"], stats[0], stats[1], training, True, part_in=part)
        m, mblob = ops.sfh_mixer_fwd(y1, mp, stats[4], stats[5], training, True)
        x1, p1 = ops.scale_res_fwd(m, xd, P[pre + "beta"], want_part=True) if training else (ops.scale_res_fwd(m, xd, P[pre + "beta"]), None)
        y2, st2 = ops.bn2d_fwd(x1, P[pre + "norm2.weight"], P[pre + "norm2.bias"], stats[2], stats[3], training, True, part_in=p1)
        f, fblob = ops.sfh_ffn_fwd(y2, fp, True)
        if training and i + 1 < len(prefixes):
            out, part = ops.scale_res_fwd(f, x1, P[pre + "gamma"], want_part=True)
        else:
            out, part = ops.scale_res_fwd(f, x1, P[pre + "gamma"]), None
        ctxs.append((pre, xd, y1, st1, m, mblob, x1, y2, st2, f, fblob, mp, fp))
        xd = out
    y, d = xd, cot.to(DEV).to(dtype)
    for pre, xin, y1, st1, m, mblob, x1, y2, st2, f, fblob, mp, fp in reversed(ctxs):
        df = ops.scale_res_bwd(f, d, P[pre + "gamma"], G[pre + "gamma"], False)
        dy2 = ops.sfh_ffn_bwd(y2, df, fp, fblob, [G[pre + "ffn." + k] for k in FR.FFN_PARAMS], False)
        dx1 = ops.bn2d_bwd(x1, dy2, P[pre + "norm2.weight"], st2, (G[pre + "norm2.weight"], G[pre + "norm2.bias"]), False, training, dres=d)
        dm = ops.scale_res_bwd(m, dx1, P[pre + "beta"], G[pre + "beta"], False)
        dy1 = ops.sfh_mixer_bwd(y1, dm, mp, mblob, [G[pre + "mixer." + k] for k in M.MIXER_PARAMS], False, training)
        d = ops.bn2d_bwd(xin, dy1, P[pre + "norm1.weight"], st1, (G[pre + "norm1.weight"], G[pre + "norm1.bias"]), False, training, dres=dx1)
    torch.cuda.synchronize()
    got = {"y": y.cpu(), "dx": d.cpu()}
    got.update({"g." + k: G[k].cpu() for k in G})
    got.update({"buf." + k: P[k].cpu() for k in R.buffers_of(kind, args)})
    return got


def _equal(a, b, keys=None):
    assert set(a) == set(b)
    bad = [k for k in (keys or a) if not (a[k].shape == b[k].shape and torch.equal(a[k], b[k]))]
    assert not bad, bad


# ------------------------------------------------------------------ 1. bitwise against the op sequence
@MODES
@DTYPES
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_node_equals_the_op_sequence_bitwise(name, dtype, training):
    """y, dx, every parameter gradient and every running statistic of the ONE node equal those of the six calls per Block made one
    by one through the parts' ops, bit for bit, in both dtypes and both modes."""
    kind, args, _, _, _ = R.CASES[name]
    sd = R.case_state(name)
    x, cot = R.case_io(name)
    got = run_native(build(kind, args, sd, training), kind, args, x, cot, dtype)
    want = op_sequence(kind, args, sd, x, cot, dtype, training)
    assert set(got) == R.tensors(kind, args) and all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    _equal(got, want)
    moved = any(not torch.equal(got["buf." + k], sd[k]) for k in R.buffers_of(kind, args))
    assert moved == training


# ------------------------------------------------------------------ 2. bitwise against the public modules under autograd
@MODES
@DTYPES
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_node_equals_the_public_module_chain(name, dtype, training):
    """BatchNorm2d -> Mixer -> scaled_residual -> BatchNorm2d -> FFN -> scaled_residual as six autograd nodes per Block: the forward
    and the running statistics are the node's bit for bit in both dtypes (part_in reproduces the statistics exactly), the backward
    in float32 (dx + dres is one rounded add either way).  In bfloat16 the chain rounds dx and the residual gradient separately
    where the seam rounds once, so the backward is held by (1) alone."""
    kind, args, _, _, _ = R.CASES[name]
    sd = R.case_state(name)
    x, cot = R.case_io(name)
    node_mod, chain_mod = build(kind, args, sd, training), build(kind, args, sd, training)
    got = run_native(node_mod, kind, args, x, cot, dtype)
    want = run_native(chain_mod, kind, args, x, cot, dtype, forward=chain)
    fwd = ["y"] + ["buf." + k for k in R.buffers_of(kind, args)]
    _equal(got, want, fwd if dtype == torch.bfloat16 else None)
    assert counters(node_mod) == counters(chain_mod) == [int(training)] * (3 * len(R.block_prefixes(kind, args)))


# ------------------------------------------------------------------ 3. the reference fixtures
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_node_matches_reference_fixture(name):
    """fp32 against the fixtures captured from the reference, at the 1e-3 of the existing fixture tests: output, dx, every parameter
    gradient and every running statistic after the call; the tensor set is the fixture's."""
    kind, args, _, _, training = R.CASES[name]
    x, cot = R.case_io(name)
    got = run_native(build(kind, args, R.case_state(name), training), kind, args, x, cot, torch.float32)
    gold = load(name)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        print(name, k, f"{check(k, v, gold, 1e-3, what=name + ' '):.3e}")


# ------------------------------------------------------------------ 4. main_grad
@pytest.mark.parametrize("name", ["sfh_block_d4", "sfh_stage_d4_n2"])
def test_main_grad_buffers_take_prefill_plus_fresh_gradients(name):
    kind, args, _, _, training = R.CASES[name]
    sd = R.case_state(name)
    x, cot = R.case_io(name)
    fresh = run_native(build(kind, args, sd, training), kind, args, x, cot, torch.float32)
    mod = build(kind, args, sd, training)
    base = {}
    for i, (k, p) in enumerate(mod.named_parameters()):
        base[k] = seeded_input(tuple(p.shape), 400 + i).to(DEV)
        p.main_grad = base[k].clone()
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg)
    y.backward(cot.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu(), fresh["y"]) and torch.equal(xg.grad.cpu(), fresh["dx"])
    for k, p in mod.named_parameters():
        assert p.grad is None, k
        assert torch.equal(p.main_grad.cpu(), base[k].cpu() + fresh["g." + k]), k


# ------------------------------------------------------------------ 5. poisoned buffers, repeated runs
def _raw(name, dtype, fill):
    """One Block forward and backward straight through the C-ABI on buffers of the test's own: workspace, saved blob, out, dx, the
    pair buffer and the gradient buffers filled with ``fill`` bytes first (0xff: NaN in either dtype)."""
    from image_restoration_amd import _lib as L
    kind, args, (B, H, W), _, training = R.CASES[name]
    assert kind == "block"
    dim = args["dim"]
    ops, lib, n = O(), L.lib(), N()
    blk = build(kind, args, R.case_state(name), training)
    params = list(n._block_params(blk))
    stats = [t for bn in n._block_norms(blk) for t in (bn.running_mean, bn.running_var)]

    def filled(nbytes):
        return torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    x, cot = R.case_io(name)
    xd, cd = x.to(DEV).to(dtype), cot.to(DEV).to(dtype)
    out, dx = (filled(xd.numel() * xd.element_size()).view(dtype).view_as(xd) for _ in range(2))
    grads = [filled(p.numel() * 4).view(torch.float32).view_as(p) for p in params]
    s = L.SfhMixerShape(B, dim, H, W, ops._dtype_code(dtype), int(training), 1e-5, 0.1)
    plan = ops.sfh_block_plan(B, dim, H, W, dtype, training)
    ws, saved, part = filled(plan["workspace"]), filled(plan["saved_bytes"]), filled(plan["pair_bytes"])
    pp = ops._sb_struct(L.SfhBlockParams, params, "parameter")
    gg = ops._sb_struct(L.SfhBlockGrads, grads, "gradient", 0)
    stt = L.SfhBlockStats(*[t.data_ptr() for t in stats])
    st = ops._stream()
    L.check(lib.mi_sfh_block_fwd(C.byref(s), C.byref(pp), xd.data_ptr(), out.data_ptr(), C.byref(stt), None, part.data_ptr(), saved.data_ptr(),
                                 ws.data_ptr(), st), "fwd")
    ws.fill_(fill)
    L.check(lib.mi_sfh_block_bwd(C.byref(s), C.byref(pp), xd.data_ptr(), cd.data_ptr(), dx.data_ptr(), C.byref(gg), saved.data_ptr(),
                                 ws.data_ptr(), st), "bwd")
    torch.cuda.synchronize()
    res = {"y": out, "dx": dx, "part": part.view(torch.float32)}
    res.update({f"g{i}": g for i, g in enumerate(grads)})
    res.update({f"s{i}": t for i, t in enumerate(stats)})
    return {k: v.cpu() for k, v in res.items()}


@DTYPES
@pytest.mark.parametrize("name", ["sfh_block_d4", "sfh_block_d6_eval", "sfh_block_d4_two_chunks"])
def test_poisoned_buffers_change_nothing_and_two_runs_are_equal(name, dtype):
    """Workspace, saved blob, out, dx, the pairs and the gradient buffers NaN-filled before the calls: no NaN comes out and the
    results equal those on zero-filled buffers bit for bit (nothing is read before it is written); a second poisoned run equals the
    first.  In eval mode the pair buffer is left alone."""
    a, b, c = _raw(name, dtype, 0xFF), _raw(name, dtype, 0), _raw(name, dtype, 0xFF)
    training = R.CASES[name][4]
    for k in a:
        if k == "part" and not training:
            assert bool(torch.isnan(a[k]).all()) and not b[k].any()
            continue
        assert bool(torch.isfinite(a[k].float()).all()), k
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert all(float(a[f"g{i}"].abs().max()) > 0 for i in range(R_PARAMS))


R_PARAMS = len(R.BLOCK_PARAMS)


# ------------------------------------------------------------------ 6. no_grad and eval mode
@DTYPES
@pytest.mark.parametrize("name", ["sfh_block_d4", "sfh_stage_d4_n2", "sfh_stage_d4_n3_eval"])
def test_no_grad_equals_grad_mode_and_eval_mode_leaves_the_buffers(name, dtype):
    kind, args, _, _, training = R.CASES[name]
    sd = R.case_state(name)
    x, cot = R.case_io(name)
    a = run_native(build(kind, args, sd, training), kind, args, x, cot, dtype)
    b = run_native(build(kind, args, sd, training), kind, args, x, cot, dtype)
    _equal(a, b)                                                   # two runs are equal
    mod = build(kind, args, sd, training)
    with torch.no_grad():
        y0 = mod(x.to(DEV).to(dtype))                              # saved == NULL: the planes live in the workspace
    assert not y0.requires_grad and y0.grad_fn is None and torch.equal(y0.cpu(), a["y"])
    after = mod.state_dict()
    nblocks = len(R.block_prefixes(kind, args))
    for k in R.buffers_of(kind, args):
        assert torch.equal(after[k].cpu(), a["buf." + k]), k       # as in grad mode
        assert torch.equal(after[k].cpu(), sd[k]) == (not training), k
    assert counters(mod) == [int(training)] * (3 * nblocks)        # training: all three counters of every Block advance by one
    if training:
        with torch.no_grad():
            mod(x.to(DEV).to(dtype))
        assert counters(mod) == [2] * (3 * nblocks)
    y = mod(x.to(DEV).to(dtype).requires_grad_(True))
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("_ModuleOpFn")      # ONE node over the whole run of blocks
    assert all(type(f[0]).__name__ == "AccumulateGrad" for f in y.grad_fn.next_functions if f[0] is not None)


# ------------------------------------------------------------------ 7. runtime refusals
def test_runtime_refusals():
    n = N()
    blk = build("block", dict(dim=4), R.make_state("block", dict(dim=4), 5))
    with pytest.raises(RuntimeError, match="MI355X only"):
        blk(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match="do not fit"):
        blk(torch.zeros(1, 6, 8, 8, device=DEV))
    with pytest.raises(NotImplementedError, match="H=1 outside"):
        blk(torch.zeros(2, 4, 1, 8, device=DEV))
    with pytest.raises(RuntimeError, match="contiguous"):
        blk(torch.zeros(1, 8, 8, 4, device=DEV).permute(0, 3, 1, 2))
    assert counters(blk) == [0, 0, 0]
    stage = n.Stage(2, 4).to(DEV)
    stage.blocks[1].eval()
    with pytest.raises(NotImplementedError, match="share one eps"):
        stage(torch.zeros(1, 4, 8, 8, device=DEV))

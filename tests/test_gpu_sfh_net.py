"""SFHformer's Backbone on the MI355X: the two tiny networks of tests/sfh_block_ref.py (widths [4, 8, 16, 8, 4], depths
[1, 1, 2, 1, 1], a 16 x 20 input, so the deepest plane is 4 x 5) bit for bit against the same glue calls with every Stage replaced by
its chain of public modules, against the reference fixtures, under no_grad and in eval mode, the runtime refusals, and one
FlatTrainer step."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import sfh_block_ref as R  # noqa: E402
from oracle.fixtures import check, load, seeded_input  # noqa: E402
from test_gpu_sfh_block import DEV, DTYPES, N, _equal, build, chain_stage, counters, run_native  # noqa: E402

pytestmark = pytest.mark.gpu
NET_CASES = [n for n, c in R.CASES.items() if c[0] == "net"]


def chain_net(net, x):
    """Backbone.forward with the same glue calls and every Stage as BatchNorm2d -> Mixer -> scaled_residual -> BatchNorm2d -> FFN ->
    scaled_residual per Block."""
    n = N()
    copy0 = x
    copy1 = x = chain_stage(net.layer1, net.patch_embed(x))
    copy2 = x = chain_stage(net.layer2, net.downsample1(x))
    x = chain_stage(net.layer3, net.downsample2(x))
    x = chain_stage(net.layer8, n._up_skip(net.upsample3, x, copy2, net.skip2))
    x = chain_stage(net.layer9, n._up_skip(net.upsample4, x, copy1, net.skip1))
    return net.patch_unembed(x, copy0)


@DTYPES
@pytest.mark.parametrize("name", NET_CASES)
def test_backbone_equals_the_public_module_chain(name, dtype):
    """Forward and running statistics bit for bit in both dtypes, the backward (dx and every parameter gradient) in float32; five
    autograd nodes for the five Stages against six per Block."""
    kind, args, _, _, training = R.CASES[name]
    sd = R.case_state(name)
    x, cot = R.case_io(name)
    node_mod, chain_mod = build(kind, args, sd, training), build(kind, args, sd, training)
    got = run_native(node_mod, kind, args, x, cot, dtype)
    want = run_native(chain_mod, kind, args, x, cot, dtype, forward=chain_net)
    assert set(got) == R.tensors(kind, args) and all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    fwd = ["y"] + ["buf." + k for k in R.buffers_of(kind, args)]
    _equal(got, want, fwd if dtype == torch.bfloat16 else None)
    assert counters(node_mod) == counters(chain_mod) == [int(training)] * (3 * len(R.block_prefixes(kind, args)))


@pytest.mark.parametrize("name", NET_CASES)
def test_backbone_matches_reference_fixture(name):
    """fp32 against the fixtures captured from the reference Backbone at 1e-3: output, dx, every parameter gradient, every running
    statistic after the call; the tensor set is the fixture's."""
    kind, args, _, _, training = R.CASES[name]
    x, cot = R.case_io(name)
    got = run_native(build(kind, args, R.case_state(name), training), kind, args, x, cot, torch.float32)
    gold = load(name)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    worst = max((check(k, v, gold, 1e-3, what=name + " "), k) for k, v in got.items())
    print(name, "worst", worst)


BF16_BAR = 0.1


@pytest.mark.parametrize("name", NET_CASES)
def test_backbone_bf16_output_matches_reference_fixture(name):
    """The bfloat16 glue (split-weight products, the shuffle into the concatenation buffer) is otherwise compared only with a chain
    that shares it: here y in bfloat16 against the reference's fixture.  The bar is a composition check, not a parity bound: every
    stored activation carries a 2^-9 rounding, the module parity tests hold one module's tensors to 3e-2 in bfloat16, and the output
    is the input plus what six Blocks in sequence add, whose errors add like independent terms, sqrt(6) x 3e-2 = 7.4e-2, taken as
    0.1; a wrong panel order or weight view is an error of order 1."""
    kind, args, _, _, training = R.CASES[name]
    x, _ = R.case_io(name)
    mod = build(kind, args, R.case_state(name), training)
    with torch.no_grad():
        y = mod(x.to(DEV).to(torch.bfloat16))
    print(name, "bf16 y", f"{check('y', y.float().cpu(), load(name), BF16_BAR, what=name + ' bf16 '):.3e}")


@DTYPES
@pytest.mark.parametrize("name", NET_CASES)
def test_backbone_no_grad_and_eval_mode(name, dtype):
    kind, args, _, _, training = R.CASES[name]
    sd = R.case_state(name)
    x, cot = R.case_io(name)
    a = run_native(build(kind, args, sd, training), kind, args, x, cot, dtype)
    mod = build(kind, args, sd, training)
    with torch.no_grad():
        y0 = mod(x.to(DEV).to(dtype))
    assert not y0.requires_grad and y0.grad_fn is None and torch.equal(y0.cpu(), a["y"])
    after = mod.state_dict()
    for k in R.buffers_of(kind, args):
        assert torch.equal(after[k].cpu(), a["buf." + k]), k
        assert torch.equal(after[k].cpu(), sd[k]) == (not training), k
    assert counters(mod) == [int(training)] * 18


def test_backbone_runtime_refusals():
    net = build("net", R.NET, R.make_state("net", R.NET, 5))
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(torch.zeros(1, 3, 16, 16))
    for hw in ((18, 20), (16, 22), (4, 16), (16, 4)):
        with pytest.raises(ValueError, match="multiples of 4, at least 8"):
            net(torch.zeros(1, 3, *hw, device=DEV))
    assert counters(net) == [0] * 18
    with torch.no_grad():
        assert net(torch.zeros(1, 3, 8, 8, device=DEV)).shape == (1, 3, 8, 8)       # the smallest input: the deepest plane is 2 x 2


def test_flat_trainer_takes_a_step_on_the_tiny_backbone():
    """One FlatTrainer step (main_grad accumulation, fused AdamW): every parameter finite, and every parameter with a non-zero
    gradient moved.  No trajectory bar: a convolution bias in front of a BatchNorm has a near-zero gradient, and AdamW turns its
    rounding into a step of random sign."""
    from image_restoration_amd.trainer import FlatTrainer
    sd0 = R.make_state("net", R.NET, 411)
    net = build("net", R.NET, sd0)
    x, tgt = seeded_input((2, 3, 16, 20), 412).to(DEV), seeded_input((2, 3, 16, 20), 413).to(DEV)
    tr = FlatTrainer(net, lr=1e-3, weight_decay=0.01)
    try:
        tr.zero_grad()
        loss = (net(x) - tgt).abs().mean()
        loss.backward()
        tr.reduce_gradients()
        grads = {k: p.main_grad.detach().cpu().clone() for k, p in net.named_parameters()}
        tr.optimizer_step()
        torch.cuda.synchronize()
        got = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    finally:
        tr.close()
    assert float(loss) == float(loss) and abs(float(loss)) < 1e6
    assert len(grads) == len(R.params_of("net", R.NET))
    for k, g in grads.items():
        assert bool(torch.isfinite(got[k]).all()) and bool(torch.isfinite(g).all()), k
        if bool(g.any()):
            assert not torch.equal(got[k], sd0[k]), k
    assert any(bool(g.any()) for g in grads.values())
    assert counters(net) == [1] * 18

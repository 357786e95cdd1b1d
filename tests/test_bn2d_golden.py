"""CPU checks of the BatchNorm2d / scaled-residual restatement (tests/bn2d_ref.py): its formula form against torch.nn.BatchNorm2d and
the reference's ``x * beta + copy`` under autograd in fp64, its device form against the formula form in fp64, the preconditions and
shapes of the parity cases, the module's state_dict against torch's, the exports, and the shape of the committed bounds table."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import bn2d_ref as R  # noqa: E402
import sfh_ref as S  # noqa: E402
from oracle.fixtures import load  # noqa: E402

MODES = {"train": True, "eval": False}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_restatement_matches_torch_in_fp64(name, mode):
    """The formulas against torch.nn.BatchNorm2d and ``x * beta + copy`` (SFHformer.py:275) under autograd, fp64 on the CPU, at 1e-12
    of each tensor's maximum (fp64 inputs, short sums): the output, dx, every parameter gradient, the running statistics after the
    call; torch's num_batches_tracked counts a training forward and no other, which is what the native module is held to on the
    GPU (tests/test_gpu_bn2d.py)."""
    training = MODES[mode]
    io = {k: v.double() for k, v in R.parity_io(name).items()}
    got = R.run(io, training)
    C = io["x"].shape[1]
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOMENTUM).double().train(training)
    bn.load_state_dict({"weight": io["w"], "bias": io["b"], "running_mean": io["rm"], "running_var": io["rv"],
                        "num_batches_tracked": torch.tensor(0)}, strict=True)
    x = io["x"].clone().requires_grad_(True)
    y = bn(x)
    y.backward(io["cot"])
    beta = io["scale"].view(1, C, 1, 1).clone().requires_grad_(True)
    f, copy = io["f"].clone().requires_grad_(True), io["x"].clone().requires_grad_(True)
    out = f * beta + copy
    out.backward(io["cot"])
    want = {"y": y.detach(), "dx": x.grad, "dw": bn.weight.grad, "db": bn.bias.grad, "rm": bn.running_mean, "rv": bn.running_var,
            "out": out.detach(), "df": f.grad, "ds": beta.grad.reshape(-1)}
    assert set(got) == set(want) == set(R.TENSORS)
    for k in R.TENSORS:
        assert got[k].shape == want[k].shape and R.rel_err(got[k], want[k]) <= 1e-12, (name, mode, k, R.rel_err(got[k], want[k]))
    assert torch.equal(copy.grad, io["cot"])                       # the gradient towards x is the cotangent itself
    assert int(bn.num_batches_tracked) == int(training)
    assert torch.equal(got["rm"], io["rm"]) == (not training)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_device_form_equals_formula_form_in_fp64(name, mode):
    """Every parity case, either vector width: the device form IS the function, to 1e-11 in every tensor."""
    io = R.parity_io(name)
    a = R.run(io, MODES[mode])
    for V in (4, 8):
        b = R.run(io, MODES[mode], device=True, V=V)
        for k in R.TENSORS:
            assert R.rel_err(b[k], a[k]) <= 1e-11, (name, mode, V, k, R.rel_err(b[k], a[k]))


def test_the_parity_cases_are_the_issues_and_keep_the_variance_floor():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import ops
    CH = ops.bn2d_plan(2, 3, 8, 8)["chunk"]
    assert CH == R.CHUNK and S.VAR_FLOOR == 1e-3 and R.VAR_FLOOR is S.VAR_FLOOR
    shapes = {n: c[0] for n, c in R.PARITY_CASES.items()}
    assert shapes["n2"] == (2, 3, 1, 1) and shapes["odd"] == (2, 3, 5, 7)
    for n, N in (("ch_m1", CH - 1), ("ch", CH), ("ch_p1", CH + 1)):
        assert shapes[n][:2] == (1, 2) and shapes[n][2] * shapes[n][3] == N
    assert shapes["ragged"][:2] == (3, 5) and shapes["ragged"][2] * shapes["ragged"][3] == 2 * CH + 8
    assert shapes["c1"] == (2, 1, 4, 4) and shapes["c257"] == (2, 257, 2, 2)
    assert shapes["dc"] == shapes["ragged"] and R.PARITY_CASES["dc"][1] == R.PARITY_CASES["ragged"][1]
    dc, plain = R.parity_io("dc")["x"], R.parity_io("ragged")["x"]
    assert torch.equal(dc, plain + R.DC_OFFSET) and R.DC_OFFSET >= 100 * float(plain.std())
    const = R.parity_io("const")["x"]
    assert bool((const[:, 1] == 2.0).all()) and float(R.channel_variances(const)[1]) == 0.0
    B, C, H, W = shapes["grid"]
    assert ops.bn2d_plan(B, C, H, W)["chunks"] > ops.bn2d_plan(B, C, H, W)["grid_chunks"] == 1 << 20
    # both access forms occur in either dtype, and the precondition holds on the input as either dtype stores it
    assert {ops.bn2d_plan(*s, torch.float32)["vector_width"] for s in shapes.values()} == {1, 4}
    assert {ops.bn2d_plan(*s, torch.bfloat16)["vector_width"] for s in shapes.values()} == {1, 8}
    for name in R.PARITY_CASES:
        x = R.parity_io(name)["x"]
        assert R.variances_ok(x) and R.variances_ok(x.bfloat16().float()), name


def test_module_has_torchs_keys_and_loads_a_checkpoint_slice():
    import torch.nn as nn
    import image_restoration_amd
    from image_restoration_amd import sfhformer as N
    for name in ("BatchNorm2d", "scaled_residual"):
        assert getattr(image_restoration_amd, name) is getattr(N, name) and name in image_restoration_amd.__all__ and name in N.__all__
    for C, kw in ((1, {}), (32, {}), (257, dict(eps=1e-3, momentum=0.2))):
        mine, ref = N.BatchNorm2d(C, **kw), nn.BatchNorm2d(C, **kw)
        assert isinstance(mine, nn.BatchNorm2d) and (mine.eps, mine.momentum) == (ref.eps, ref.momentum)
        a, b = mine.state_dict(), ref.state_dict()
        assert list(a) == list(b) == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
        assert [(v.shape, v.dtype) for v in a.values()] == [(v.shape, v.dtype) for v in b.values()]
        assert [k for k, _ in mine.named_parameters()] == ["weight", "bias"]
        assert [k for k, _ in mine.named_buffers()] == [k for k, _ in ref.named_buffers()]
        state = {"weight": torch.randn(C), "bias": torch.randn(C), "running_mean": torch.randn(C), "running_var": torch.rand(C) + 0.5,
                 "num_batches_tracked": torch.tensor(7)}
        mine.load_state_dict(state, strict=True)
        assert all(torch.equal(mine.state_dict()[k], v) for k, v in state.items())
    for kw in (dict(affine=False), dict(track_running_stats=False), dict(momentum=None)):
        with pytest.raises(NotImplementedError, match="fixed momentum"):
            N.BatchNorm2d(8, **kw)
    for bad in (0, 4097, -1, 8.0):
        with pytest.raises(NotImplementedError, match="not covered"):
            N.BatchNorm2d(bad)
    N.BatchNorm2d(4096)


def test_bounds_table_has_one_scalar_per_case_dtype_mode_and_tensor():
    """The committed table is what tools/bn2d_bounds.py writes: its keys and their sizes are checked, nothing is recomputed here (a
    recomputed fp32 figure is one realisation of rounding noise; the tool's sums are explicit and ordered, so the table does not
    depend on the host, but no test rests on that)."""
    bounds = load("bn2d_bounds")
    want = {f"{n}.{t}.{m}.{k}" for n in R.PARITY_CASES for t in ("fp32", "bf16") for m in MODES for k in R.TENSORS}
    assert set(bounds.files) == want
    for key in want:
        v = bounds[key]
        assert v.shape == () and 0 <= float(v) < (2e-4 if ".fp32." in key else 0.1), key
    for n in R.PARITY_CASES:
        for m in MODES:
            for k in ("y", "dx", "out", "df"):             # set by the bf16 storage rounding, 2^-9-sized
                assert 5e-4 < float(bounds[f"{n}.bf16.{m}.{k}"]) < 2e-2, (n, m, k)

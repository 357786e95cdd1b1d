"""CPU checks of the FourierUnit restatement (tests/sfh_ref.py): its torch.fft form against the fixtures captured from the reference
(tools/capture_golden_fourier_unit.py), its dense form (the device's formulation: planar channels, statistics of the unscaled
spectrum, the folded grouped conv) against the torch.fft form in fp64, the parity cases' variance precondition, the key list against
the module's state_dict, and the committed bounds table against what tools/sfh_bounds.py computes."""
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import sfh_ref as R  # noqa: E402
from oracle.fixtures import check, load  # noqa: E402


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_fourier_unit",
                                                  os.path.join(ROOT, "tools", "capture_golden_fourier_unit.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()
TENSORS = {"y", "dx", "rm", "rv"} | {"g." + k for k in R.PARAMS}


@pytest.mark.parametrize("dense", [False, True], ids=["fft", "dense"])
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_reference_fixture(name, dense):
    """Both forms on the float32 state and inputs, at the bar of the FreMLP golden test (1e-9, evaluated in fp64), and in float32
    arithmetic at float32's own bar; the fixtures hold the running statistics after the step (eval: unchanged)."""
    c, groups, bhw, seed, training = G.CASES[name]
    gold = load(name)
    x, cot = G.case_io(c, bhw, seed)
    sd = G.case_state(c, groups, seed, training)
    got = R.run(x, cot, sd, groups, training, dense=dense)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got) == TENSORS, f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        check(k, v, gold, 1e-9, what=name + " ")
    assert all(float(v.abs().max()) > 0 for v in got.values())
    if not training:
        assert torch.equal(got["rm"], sd["bn.running_mean"].double()) and torch.equal(got["rv"], sd["bn.running_var"].double())
    for k, v in R.run(x, cot, sd, groups, training, torch.float32, dense=dense).items():
        check(k, v, gold, 1e-4, what=name + " fp32 ")


@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_dense_form_equals_fft_form_in_fp64(name):
    """Every parity case: the dense form IS the function, to 1e-11 in every tensor (the fold, the planar permutation and the scale
    folded into the statistics change nothing); and the recorded seed keeps the variance precondition in both storage precisions:
    every spectral channel's batch variance is exactly 0 or at least 1e-3 of the median channel's."""
    sd, x, cot, groups, training = R.parity_io(name)
    for dtype in (torch.float32, torch.bfloat16):
        assert R.variances_ok(R.storage_io(x, cot, dtype)[0]), (name, dtype)
    a, b = R.run(x, cot, sd, groups, training), R.run(x, cot, sd, groups, training, dense=True)
    assert set(a) == set(b) == TENSORS
    for k in a:
        assert R.rel_err(b[k], a[k]) <= 1e-11, (name, k, R.rel_err(b[k], a[k]))


def test_the_special_cases_are_what_their_names_say():
    """zero: two spectral channels with batch variance exactly 0; dc: the DC bin of every Re plane dwarfs the other bins; g1: the
    gate is exactly 1 (its parameters get exactly zero gradient); eval: the seeded running statistics are not the fresh ones."""
    _, x, _, _, _ = R.parity_io("zero")
    v = R.channel_variances(x)
    assert int((v == 0).sum()) == 2 and float(v[2]) == 0 and float(v[3]) == 0
    _, x, _, _, _ = R.parity_io("dc")
    z = torch.fft.rfft2(x.double(), norm="ortho").real
    rest = z.clone()
    rest[:, :, 0, 0] = 0
    assert float(z[:, :, 0, 0].abs().min()) > 50 * float(rest.pow(2).mean().sqrt())   # one bin carries the channel's sum AND its sum of squares
    sd, x, cot, groups, training = R.parity_io("g1")
    got = R.run(x, cot, sd, groups, training)
    assert float(got["g.weight.0.weight"].abs().max()) == 0 and float(got["g.weight.0.bias"].abs().max()) == 0
    sd = R.parity_io("eval")[0]
    assert float(sd["bn.running_mean"].abs().min()) > 0 and float((sd["bn.running_var"] - 1).abs().min()) > 0


def test_module_has_the_reference_keys_and_loads_a_checkpoint_slice():
    from image_restoration_amd import sfhformer as N
    import image_restoration_amd
    assert image_restoration_amd.FourierUnit is N.FourierUnit and "FourierUnit" in image_restoration_amd.__all__
    keys = load("sfh_fu_keys")
    for tag, args in G.KEY_CASES:
        mod = N.FourierUnit(**args)
        sd = mod.state_dict()
        assert list(sd) == [str(k) for k in keys[tag + ".keys"]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys[tag + ".shapes"]]
        assert [k for k, _ in mod.named_buffers()] == [str(k) for k in keys[tag + ".buffers"]]
        c, groups = args["in_channels"], args.get("groups", 4)
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.state_dict_layout(c, groups)
        mod.load_state_dict(R.module_state(R.make_state(c, groups, 5, trivial_stats=False), steps=3), strict=True)
        assert int(mod.bn.num_batches_tracked) == 3
    assert list(sd) == ["bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked", "fdc.weight", "fdc.bias",
                        "weight.0.weight", "weight.0.bias", "fpe.weight", "fpe.bias"]


def test_bounds_table_is_the_host_error_of_the_dense_form():
    """The committed bounds are what tools/sfh_bounds.py computes (three cheap cases recomputed here), one entry per case, dtype and
    tensor; bf16 storage costs y and dx 2^-9-sized errors and leaves the fp32 tensors at fp32 size; eval leaves the running
    statistics exactly alone (bound 0)."""
    bounds = load("sfh_fu_bounds")
    for name in ("odd", "g2", "zero"):
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            errs, _ = R.host_errors(name, dtype)
            for k, v in errs.items():
                assert v / 3 <= float(bounds[f"{name}.{tag}.{k}"]) <= 3 * v, (name, tag, k)   # (summation order varies by host)
    for name in R.PARITY_CASES:
        for tag in ("fp32", "bf16"):
            assert all(0 <= float(bounds[f"{name}.{tag}.{k}"]) < 0.05 for k in TENSORS), (name, tag)
            assert all(float(bounds[f"{name}.{tag}.{k}"]) < 1e-4 for k in TENSORS - {"y", "dx"}), (name, tag)
        assert all(float(bounds[f"{name}.fp32.{k}"]) < 1e-4 for k in TENSORS), name
    assert float(bounds["eval.fp32.rm"]) == 0 and float(bounds["eval.bf16.rv"]) == 0
    assert len(bounds.files) == len(R.PARITY_CASES) * 2 * len(TENSORS)

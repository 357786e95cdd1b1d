"""CPU checks of DarkIR's FreMLP restatement (tests/fremlp_ref.py): its torch.fft form against the fixtures captured from the
reference (tools/capture_golden_fremlp.py), its dense form (the device's formulation) against the torch.fft form in fp64, the
zero-spectrum convention in both forms, and the committed bounds table against what tools/fremlp_bounds.py computes."""
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import fremlp_ref as R  # noqa: E402
from oracle.fixtures import check, load  # noqa: E402


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_fremlp", os.path.join(ROOT, "tools", "capture_golden_fremlp.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_reference_fixture(name):
    """The torch.fft form on the float32 state and inputs, at the bar of the DBlock golden test (1e-9: evaluated in fp64, as
    there; float32 arithmetic could not meet that bar), and in float32 arithmetic at float32's own bar."""
    nc, expand, bhw, seed = G.CASES[name]
    gold = load(name)
    x, cot = G.case_io(nc, bhw, seed)
    sd = R.make_state(R.fremlp_shapes(nc, expand), seed)
    got = R.run(x, cot, sd)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        check(k, v, gold, 1e-9, what=name + " ")
    assert all(float(v.abs().max()) > 0 for v in got.values())
    for k, v in R.run(x, cot, sd, torch.float32).items():
        check(k, v, gold, 1e-4, what=name + " fp32 ")


@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_dense_form_equals_fft_form_in_fp64(name):
    """Every parity case (the largest takes a second): the dense form IS the function, to 1e-12 in every tensor; and the case's
    recorded seed keeps the spectrum off zero in both storage precisions."""
    sd, x, cot, _ = R.parity_io(name)
    for dtype in (torch.float32, torch.bfloat16):
        assert R.spectrum_floor(R.storage_io(x, cot, dtype)[0]) >= R.FLOOR, (name, dtype)
    a, b = R.run(x, cot, sd), R.run(x, cot, sd, dense=True)
    assert set(a) == set(b)
    for k in a:
        assert R.rel_err(b[k], a[k]) <= 1e-12, (name, k, R.rel_err(b[k], a[k]))


@pytest.mark.parametrize("dense", [False, True], ids=["fft", "dense"])
def test_zero_sample_gives_a_scaled_delta_and_no_input_gradient(dense):
    """Z = 0 everywhere: angle = 0 (u = (1, 0)), so out = m delta at pixel (0, 0), m = W2 LeakyReLU(b1) + b2; abs and angle have
    zero gradient at 0, so dx = 0 for that sample; the parameter gradients are not zero."""
    (B, nc, H, W), expand, _ = R.PARITY_CASES["expand3"]
    sd, x, cot, _ = R.parity_io("expand3")
    x[1] = 0
    got = R.run(x, cot, sd, dense=dense)
    p = {k: v.double() for k, v in sd.items()}
    m = p["process1.2.weight"].flatten(1) @ torch.nn.functional.leaky_relu(p["process1.0.bias"], 0.1) + p["process1.2.bias"]
    want = torch.zeros(nc, H, W, dtype=torch.float64)
    want[:, 0, 0] = m
    assert R.rel_err(got["y"][1], want) <= 1e-13
    assert torch.equal(got["dx"][1], torch.zeros_like(got["dx"][1]))
    assert float(got["dx"][0].abs().max()) > 0
    assert all(float(got[k].abs().max()) > 0 for k in got if k.startswith("g."))
    # the zero sample alone still reaches the biases and W2 (through LeakyReLU(b1)); W1's gradient is dh mag^T = 0
    alone = R.run(x[1:], cot[1:], sd, dense=dense)
    for k in alone:
        if k.startswith("g."):
            assert (float(alone[k].abs().max()) > 0) == (k != "g.process1.0.weight"), k


def test_c2r_dense_is_irfft2_for_any_input():
    """The inverse formula with its column weights equals irfft2 for a spectrum that is NOT Hermitian (random imaginary parts in
    the edge columns), even and odd W."""
    g = torch.Generator().manual_seed(7)
    for H, W in ((6, 8), (5, 7), (2, 2), (4, 3)):
        K = W // 2 + 1
        yre, yim = torch.randn(2, 3, H, K, generator=g, dtype=torch.float64), torch.randn(2, 3, H, K, generator=g, dtype=torch.float64)
        want = torch.fft.irfft2(torch.complex(yre, yim), s=(H, W))
        assert R.rel_err(R.c2r_dense(yre, yim, W), want) <= 1e-13, (H, W)
        x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
        zre, zim = R.r2c_dense(x)
        assert R.rel_err(torch.stack([zre, zim], -1), torch.view_as_real(torch.fft.rfft2(x))) <= 1e-13, (H, W)


def test_bounds_table_is_the_host_error_of_the_dense_form():
    """The committed bounds are what tools/fremlp_bounds.py computes (three cheap cases recomputed here), one entry per case, dtype
    and tensor; bf16 storage costs y and dx 2^-9-sized errors and leaves the fp32 parameter gradients at fp32 size."""
    bounds = load("fremlp_bounds")
    for name in ("odd", "expand1", "thin_h"):
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            errs, _ = R.host_errors(name, dtype)
            for k, v in errs.items():
                assert v / 3 <= float(bounds[f"{name}.{tag}.{k}"]) <= 3 * v, (name, tag, k)   # (summation order varies by host)
    for name, ((B, nc, H, W), expand, _) in R.PARITY_CASES.items():
        keys = ["y", "dx"] + ["g." + k for k in R.fremlp_shapes(nc, expand)]
        for tag in ("fp32", "bf16"):
            assert all(0 <= float(bounds[f"{name}.{tag}.{k}"]) < 0.05 for k in keys), (name, tag)
        assert all(float(bounds[f"{name}.fp32.{k}"]) < 1e-3 for k in keys), name

"""CPU checks of the SFHformer TokenMixer_For_Gloal / Mixer restatement (tests/sfh_mixer_ref.py): both of its forms against the
fixtures captured from the reference (tools/capture_golden_sfh_mixer.py), its device form against the formula form in fp64, the
preconditions of the parity cases, the key lists against the modules' state_dicts, the exports, and the committed bounds table."""
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import sfh_mixer_ref as R  # noqa: E402
import sfh_ref as S  # noqa: E402
from oracle.fixtures import load  # noqa: E402


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_sfh_mixer", os.path.join(ROOT, "tools", "capture_golden_sfh_mixer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


@pytest.mark.parametrize("device", [False, True], ids=["formula", "device"])
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_reference_fixture(name, device):
    """Both forms on the float32 state and inputs, at 1e-9 evaluated in fp64 and at 1e-4 in float32 arithmetic; every tensor of the
    fixture (y, dx, every parameter gradient, the running statistics afterwards) is present and non-zero."""
    kind, dim, bhw, seed, training = G.CASES[name]
    gold = load(name)
    x, cot = G.case_io(dim, bhw, seed)
    sd = G.case_state(kind, dim, seed, training)
    got = R.run(kind, x, cot, sd, training, device=device)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got) == R.tensors(kind), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        R.check(k, v, gold, 1e-9, what=name + " ")
    assert all(float(v.abs().max()) > 0 for v in got.values())
    for k, v in R.run(kind, x, cot, sd, training, torch.float32, device=device).items():
        R.check(k, v, gold, 1e-4, what=name + " fp32 ")


def test_the_fixtures_are_small_and_cover_eval_mode_and_dim_32():
    assert 4 <= len(G.CASES) <= 5
    assert any(not c[4] for c in G.CASES.values()) and any(c[1] == 32 and c[0] == "mixer" for c in G.CASES.values())
    assert {c[0] for c in G.CASES.values()} == {"mixer", "global"}
    for name in G.CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 128 * 1024, name


@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_device_form_equals_formula_form_in_fp64(name):
    """Every parity case: the device form IS the function, to 1e-11 in every tensor."""
    kind, sd, x, cot, training = R.parity_io(name)
    a, b = R.run(kind, x, cot, sd, training), R.run(kind, x, cot, sd, training, device=True)
    assert set(a) == set(b) == R.tensors(kind)
    for k in a:
        assert R.rel_err(b[k], a[k]) <= 1e-11, (name, k, R.rel_err(b[k], a[k]))


@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_preconditions_hold_for_every_parity_case(name):
    """The FourierUnit's input p keeps sfh_ref's variance floor (in both storage precisions of the module's input), and every hidden
    pre-activation of the channel attention is at least 8x its bf16 host-model error away from ReLU's kink."""
    assert S.VAR_FLOOR == 1e-3 and R.HIDDEN_MARGIN == 8.0
    ok, margin = R.preconditions(name)
    assert ok and margin >= R.HIDDEN_MARGIN, (name, ok, margin)
    assert (margin == float("inf")) == (R.PARITY_CASES[name][0] == "global")


def test_the_parity_cases_are_the_issues_and_reach_the_pool_seam():
    want = {"tiny": (1, 2, 4, 4), "odd": (2, 6, 9, 11), "tile_plus_1": (1, 4, 17, 65), "b3": (3, 8, 16, 64), "ragged": (1, 4, 40, 70),
            "deep": (2, 64, 8, 8), "wide": (1, 128, 4, 6), "odd_eval": (2, 6, 9, 11), "b3_eval": (3, 8, 16, 64), "glo_odd": (2, 3, 9, 11),
            "glo_b3": (3, 8, 16, 64), "glo_wide": (1, 128, 4, 6), "glo_eval": (2, 3, 9, 11)}
    for name, shape in want.items():
        kind, got, _, training = R.PARITY_CASES[name]
        assert got == shape and kind == ("global" if name.startswith("glo_") else "mixer") and training == (not name.endswith("eval")), name
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import ops
    pools = {n: ops.sfh_mixer_plan(*c[1])["pool"] for n, c in R.PARITY_CASES.items() if c[0] == "mixer"}
    assert pools["pool2"] == 2 and all(v == 1 for n, v in pools.items() if n != "pool2")
    assert {c[1][2] * c[1][3] % 4 == 0 for c in R.PARITY_CASES.values()} == {True, False}      # 4-wide rows and element rows


def test_modules_have_the_reference_keys_and_load_a_checkpoint_slice():
    from image_restoration_amd import sfhformer as N
    import image_restoration_amd
    for cls in ("TokenMixer_For_Gloal", "Mixer"):
        assert getattr(image_restoration_amd, cls) is getattr(N, cls) and cls in image_restoration_amd.__all__ and cls in N.__all__
    keys = load("sfh_mixer_keys")
    assert len(G.KEY_CASES) == 4
    for tag, kind, args in G.KEY_CASES:
        mod = getattr(N, G.CLASSES[kind])(**args)
        sd = mod.state_dict()
        assert list(sd) == [str(k) for k in keys[tag + ".keys"]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys[tag + ".shapes"]]
        buffers = [k for k, _ in mod.named_buffers()]
        assert buffers == [str(k) for k in keys[tag + ".buffers"]] and len(buffers) == 3
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.state_dict_layout(kind, args["dim"])
        assert [k for k, _ in mod.named_parameters()] == list(R.PARAMS[kind])
        state = R.module_state(kind, R.make_state(kind, args["dim"], 5, trivial_stats=False), steps=3)
        mod.load_state_dict(state, strict=True)
        assert all(torch.equal(mod.state_dict()[k], v) for k, v in state.items())
    mix = N.Mixer(8)
    assert isinstance(mix.mixer_gloal.FFC, N.FourierUnit) and isinstance(mix.mixer_local, N.TokenMixer_For_Local)
    assert [type(m).__name__ for m in mix.ca] == ["AdaptiveAvgPool2d", "Conv2d", "ReLU", "Conv2d", "Sigmoid"]
    with pytest.raises(NotImplementedError, match="default token mixers"):
        N.Mixer(8, token_mixer_for_local=N.FFN)
    with pytest.raises(NotImplementedError, match="default token mixers"):
        N.Mixer(8, token_mixer_for_gloal=N.TokenMixer_For_Local)


def test_bounds_table_is_the_host_error_of_the_device_form():
    """The committed bounds are what tools/sfh_mixer_bounds.py computes, one entry per case, dtype and tensor.  Recomputed here for
    three cheap cases and compared where the figure is a property of the model and not of the host: the bf16 errors of y and dx are
    set by the storage roundings (2^-9-sized, the same on every host to a few per cent).  An fp32 entry, and a bf16 entry of a
    gradient that sums few values, is one realisation of rounding noise that follows the host's summation order (a factor of 5
    between two hosts has been seen on a bias gradient), so those are held to their size only: fp32 entries are of fp32 size."""
    bounds = load("sfh_mixer_bounds")
    for name in ("tiny", "odd_eval", "glo_odd"):
        errs, _ = R.host_errors(name, torch.bfloat16)
        for k in ("y", "dx"):
            assert errs[k] / 1.5 <= float(bounds[f"{name}.bf16.{k}"]) <= 1.5 * errs[k], (name, k, errs[k])
        errs, _ = R.host_errors(name, torch.float32)
        assert all(0 <= v < 2e-5 for v in errs.values()), (name, errs)
    n = 0
    for name, (kind, _, _, _) in R.PARITY_CASES.items():
        for k in R.tensors(kind):
            assert 0 <= float(bounds[f"{name}.fp32.{k}"]) < 2e-5, (name, k)
            assert 0 <= float(bounds[f"{name}.bf16.{k}"]) < 0.1, (name, k)
            n += 2
        assert 1e-3 < float(bounds[f"{name}.bf16.y"]) < 2e-2 and 1e-3 < float(bounds[f"{name}.bf16.dx"]) < 2e-2, name
    assert len(bounds.files) == n

"""CPU checks of DRSformer's MEFC and whole network: the fp64 restatement (tests/drs_net_ref.py) against the fixtures captured from
the reference (tools/capture_golden_drs_net.py), the native modules' state_dict keys, shapes and parameter count against the
reference's, reference-shaped checkpoints loading with strict=True, and the MEFC sizing entry points without a GPU."""
import ctypes as C
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import drs_net_ref as R  # noqa: E402
import drs_ref as D  # noqa: E402
from oracle.fixtures import load  # noqa: E402


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_drs_net", os.path.join(ROOT, "tools", "capture_golden_drs_net.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


def run_ref(name):
    from image_restoration_amd import configs
    kind, dim, layer_num, steps, bhw, seed = G.CASES[name]
    shapes = G.case_shapes(kind, dim, layer_num, steps)
    sd = {k: v.double().requires_grad_(True) for k, v in D.make_state(shapes, seed).items()}
    x, cot = G.case_io(kind, dim, bhw, seed)
    x = x.double().requires_grad_(True)
    if kind == "mefc":
        y, ws = R.subnet(x, sd, layer_num, steps)
    else:
        y = R.drsformer(x, sd, configs.DRSFORMER_TINY)
        ws = None
    y.backward(cot.double())
    return y, x.grad, {k: v.grad for k, v in sd.items()}, ws


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_reference_fixture(name):
    gold = load(name)
    y, dx, grads, ws = run_ref(name)
    R.check_packed("y", y, gold, 1e-9, what=name + " ")
    R.check_packed("dx", dx, gold, 1e-9, what=name + " ")
    R.check_grads(grads, gold, 1e-9, what=name + " ")
    if ws is not None:
        for i, w in enumerate(ws):
            R.check_packed(f"w{i}", w, gold, 1e-9, what=name + " ")


def test_drsformer_state_dict_matches_reference_and_loads_strict():
    from image_restoration_amd import configs
    from image_restoration_amd.drsformer import DRSformer
    gold = load("drs_net_keys")
    keys = [str(k) for k in gold["keys"]]
    shapes = [tuple(int(d) for d in str(s).split(",")) for s in gold["shapes"]]
    net = DRSformer()
    sd = net.state_dict()
    assert list(sd) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert sum(p.numel() for p in net.parameters()) == int(gold["params"])
    assert list(R.drsformer_shapes(configs.DRSFORMER_BASE).items()) == list(zip(keys, shapes))
    # a checkpoint with the reference's keys and shapes loads unchanged
    ckpt = {k: torch.full(s, 0.5) for k, s in zip(keys, shapes)}
    net.load_state_dict(ckpt, strict=True)
    assert float(net.refinement.layers[1]._ops[3]._out[0].weight.detach().flatten()[0]) == 0.5
    tiny = DRSformer(**configs.DRSFORMER_TINY)
    tiny.load_state_dict(D.make_state(R.drsformer_shapes(configs.DRSFORMER_TINY), 1), strict=True)


def test_subnet_keys_hold_for_two_layer_pairs():
    from image_restoration_amd.drsformer import subnet
    gold = load("drs_net_keys")
    net = subnet(12, layer_num=2, steps=2)
    assert list(net.state_dict()) == [str(k) for k in gold["subnet_l2s2.keys"]]
    assert list(net.state_dict()) == list(R.subnet_shapes(12, 2, 2))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(R.subnet_shapes(12, 2, 2))


def test_mefc_sizing_and_refusals_without_gpu(lib):
    from image_restoration_amd import drsformer as N
    from image_restoration_amd import ops
    L = lib
    saved, ws = ops.mefc_sizes(2, 48, 16, 16, torch.float32, 4)
    # per step at least s, D1, U, Z and pre: 18 C-planes
    assert saved >= 4 * 18 * 2 * 48 * 256 * 4 and ws > 0
    assert ops.mefc_sizes(2, 48, 16, 16, torch.bfloat16, 4)[0] < saved
    for bad in (L.MefcShape(2, 300, 8, 8, L.MI_F32, 4), L.MefcShape(2, 48, 8, 8, L.MI_F32, 0),
                L.MefcShape(2, 48, 8, 8, L.MI_F32, 17), L.MefcShape(2, 48, 0, 8, L.MI_F32, 4)):
        assert L.lib().mi_mefc_saved_bytes(C.byref(bad)) == 0
        assert L.lib().mi_mefc_workspace(C.byref(bad)) == 0
    assert L.lib().mi_mefc_fwd(None, None, None, None, None, None, None) == -1
    with pytest.raises(RuntimeError, match="MI355X only"):
        N.subnet(16)(torch.zeros(1, 16, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        N.DRSformer(dim=16, num_blocks=[1, 1, 1, 1])(torch.zeros(1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="inside subnet"):
        N.OALayer(16, 4, 8)(torch.zeros(1, 16, 8, 8))

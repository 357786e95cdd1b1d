"""CPU checks of DarkIR's encoder block and network: the fp64 restatement (tests/eblock_ref.py) against the fixtures captured from
the reference (tools/capture_golden_eblock.py), the bounds table against the host model it is made from, the spectral floor of
every recorded seed, the training seed, and the native modules' state_dict against the reference's key lists."""
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import eblock_ref as E  # noqa: E402
from oracle.fixtures import check, load  # noqa: E402


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_eblock", os.path.join(ROOT, "tools", "capture_golden_eblock.py"))
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


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_reference_fixture(name):
    """To fp32 storage (the fixtures keep float32 subsets): 1e-6 of each tensor's largest element."""
    c, dil, extra, bhw, seed = G.CASES[name]
    gold = load(name)
    x, cot = G.case_io(c, bhw, seed)
    probe = []
    got = E.run(x, cot, E.make_state(E.eblock_shapes(c, len(dil), extra), seed), dil, probe=probe)
    assert E.floor_margin(probe) >= E.FLOOR
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        check(k, v, gold, 1e-6, what=name + " ")
    # both halves are live: beta and gamma are non-zero, so every gradient is
    assert all(float(v.abs().max()) > 0 for v in got.values())
    # the dense form of FreMLP is the same function
    dense = E.run(x, cot, E.make_state(E.eblock_shapes(c, len(dil), extra), seed), dil, dense=True)
    assert all(E.rel_err(dense[k], got[k]) < 1e-8 for k in got)


def test_network_restatement_matches_reference_fixture():
    gold = load(G.NET_CASE)
    sd, x, cots = E.net_io()
    probe = []
    got = E.run_net(x, cots, sd, E.SMALL_NET, probe=probe)
    assert len(probe) == 3 and E.floor_margin(probe) >= E.FLOOR
    assert got["y"].shape == x.shape and tuple(got["side"].shape) == (2, 3, 5, 7)       # 18 x 27 padded to 20 x 28, two levels down
    assert {k[:-4] for k in gold.files if k.endswith(".sub")} == set(got)
    for k, v in got.items():
        check(k, v, gold, 1e-6, what="net ")
    assert all(float(v.abs().max()) > 0 for v in got.values())


def test_bounds_table_is_the_host_error_of_the_restatement():
    """The committed bounds are what tools/eblock_bounds.py computes (two cheap cases recomputed here), one entry per case, dtype
    and tensor, and every recorded seed keeps the spectral floor."""
    bounds = load("eblock_bounds")
    for name in ("tiny", "sub_halo"):
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            errs, _, margin = E.host_errors(name, dtype)
            assert margin >= E.FLOOR
            for k, v in errs.items():
                assert v / 3 <= float(bounds[f"{name}.{tag}.{k}"]) <= 3 * v, (name, tag, k)   # (summation order varies by host)
    for name, (shape, dil, extra, _) in E.PARITY_CASES.items():
        keys = ["y", "dx"] + ["g." + k for k in E.eblock_shapes(shape[1], len(dil), extra)]
        for tag in ("fp32", "bf16"):
            assert all(float(bounds[f"{name}.{tag}.{k}"]) > 0 for k in keys), (name, tag)
            assert all(float(bounds[f"{name}.fp32.{k}"]) < 1e-3 for k in keys), name
    keys = ["side", "y", "dx"] + ["g." + k for k in E.net_shapes(E.SMALL_NET)]
    assert all(float(bounds[f"net.fp32.{k}"]) > 0 for k in keys)
    # (bf16: ending.bias' gradient is a sum of 972 bf16 cotangents, exact in fp32: its bound is 0 and the device has to be exact)
    assert all(float(bounds[f"net.bf16.{k}"]) >= 0 for k in keys) and float(bounds["net.bf16.g.ending.bias"]) == 0
    assert len(bounds.files) == 2 * (len(keys) + sum(2 + len(E.eblock_shapes(s[1], len(d), e)) for s, d, e, _ in E.PARITY_CASES.values()))


@pytest.mark.parametrize("name", [n for n in E.PARITY_CASES if n not in ("tiny", "sub_halo")])
def test_parity_seeds_keep_the_spectral_floor(name):
    (B, c, H, W), dil, extra, _ = E.PARITY_CASES[name]
    sd, x, cot, _ = E.parity_io(name)
    for dtype in (torch.float32, torch.bfloat16):
        xs, _ = E.storage_io(x, cot, dtype)
        probe = []
        with torch.no_grad():
            E.eblock(xs.double(), {k: v.double() for k, v in sd.items()}, dil, probe=probe)
        assert E.floor_margin(probe) >= E.FLOOR, (name, dtype, E.floor_margin(probe))


def test_training_seed_meets_the_bars_on_the_fp32_host():
    """The trajectory bars of the GPU training test are met by the fp32 host restatement (dense FreMLP) against fp64 + torch.fft:
    what the GPU test then measures is the device, not the seed."""
    sd0, x, tgt = E.train_io()
    ref_losses, ref = E.train_reference(sd0, x, tgt)
    losses, got = E.train_reference(sd0, x, tgt, torch.float32, dense=True)
    assert not E.trajectory_misses(losses, got, ref_losses, ref, sd0)
    # and the bars are not vacuous: a trajectory that never moves misses them
    assert E.trajectory_misses(losses, {k: v.clone() for k, v in sd0.items()}, ref_losses, ref, sd0)


def test_native_modules_have_reference_keys_and_refuse_cpu(lib):
    from image_restoration_amd import darkir as N
    import image_restoration_amd
    assert image_restoration_amd.EBlock is N.EBlock and image_restoration_amd.DarkIR is N.DarkIR
    keys = load("darkir_net_keys")
    for tag, args, shapes in (("eblock_extra", dict(c=32, extra_depth_wise=True), E.eblock_shapes(32, 1, True)),
                              ("eblock_dil149_plain", dict(c=16, dilations=[1, 4, 9]), E.eblock_shapes(16, 3, False))):
        blk = N.EBlock(**args)
        sd = blk.state_dict()
        assert list(sd) == [str(k) for k in keys[tag + ".keys"]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys[tag + ".shapes"]]
        blk.load_state_dict(E.make_state(shapes, seed=5))
    with pytest.raises(RuntimeError, match="MI355X only"):
        blk(torch.zeros(1, 16, 8, 8))
    net = N.DarkIR()
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in keys["darkir_m.keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys["darkir_m.shapes"]]
    net.load_state_dict(E.make_state(E.net_shapes(E.net_config()), seed=6), strict=True)
    assert isinstance(net.encoders[0], N.CustomSequential) and isinstance(net.encoders[0].modules_list[0], N.EBlock)
    assert all(b._dilations == (1,) for enc in net.encoders for b in enc.modules_list)           # EBlocks keep the default [1]
    assert all(b._dilations == (1, 4, 9) for dec in net.decoders for b in dec.modules_list)
    assert net.padder_size == 8
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(torch.zeros(1, 3, 16, 16), side_loss=True, use_adapter=None)
    small = N.DarkIR(**E.SMALL_NET)
    assert [(k, tuple(v.shape)) for k, v in small.state_dict().items()] == list(E.net_shapes(E.SMALL_NET).items())
    # refusals at construction
    with pytest.raises(NotImplementedError, match="c = 512.*c <= 256"):
        N.DarkIR(width=64)
    with pytest.raises(NotImplementedError, match="DW_Expand = 2"):
        N.EBlock(16, DW_Expand=1)
    with pytest.raises(NotImplementedError, match="1 <= c <= 256"):
        N.EBlock(257)
    for dil in ([0], [17], [1, 2, 3, 4, 5], []):
        with pytest.raises(NotImplementedError, match="1..16|1..4"):
            N.EBlock(16, dilations=dil)

"""CPU checks of the SFHformer Block / Stage / Backbone restatement (tests/sfh_block_ref.py) against the fixtures captured from the
reference (tools/capture_golden_sfh_block.py), of the modules' state_dict keys and shapes against the reference's, and of the
constructor refusals.  No device is touched."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import sfh_block_ref as R  # noqa: E402
from oracle.fixtures import check, load  # noqa: E402


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_reference_fixture(name):
    """The composition of the existing formulas on the float32 state and inputs, at 1e-9 evaluated in fp64 and at 1e-4 in float32
    arithmetic (the bars of test_sfh_mixer_golden.py); every tensor of the fixture (y, dx, every parameter gradient, every running
    statistic afterwards) is present and non-zero."""
    kind, args, _, _, training = R.CASES[name]
    gold = load(name)
    x, cot = R.case_io(name)
    sd = R.case_state(name)
    got = R.run(kind, args, x, cot, sd, training)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got) == R.tensors(kind, args), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        check(k, v, gold, 1e-9, what=name + " ")
    assert all(float(v.abs().max()) > 0 for v in got.values())
    for k, v in R.run(kind, args, x, cot, sd, training, torch.float32).items():
        check(k, v, gold, 1e-4, what=name + " fp32 ")


def test_the_cases_are_the_issues_and_beta_gamma_are_of_order_one():
    want = {"sfh_block_d4": ("block", 4, (2, 9, 11), True), "sfh_block_d6_eval": ("block", 6, (2, 8, 10), False),
            "sfh_block_d32": ("block", 32, (1, 12, 16), True), "sfh_block_d4_two_chunks": ("block", 4, (1, 72, 64), True),
            "sfh_stage_d4_n2": ("stage", 4, (2, 9, 11), True), "sfh_stage_d4_n3_eval": ("stage", 4, (2, 9, 11), False),
            "sfh_net_tiny": ("net", 4, (2, 16, 20), True), "sfh_net_tiny_eval": ("net", 4, (2, 16, 20), False)}
    assert list(R.CASES) == list(want)
    for name, (kind, dim, bhw, training) in want.items():
        k, args, shape, _, tr = R.CASES[name]
        first = args["dim"] if k == "block" else args["in_channels"] if k == "stage" else args["embed_dim"][0]
        assert (k, first, shape, tr) == (kind, dim, bhw, training), name
        sd = R.case_state(name)
        scales = [v for key, v in sd.items() if key.rsplit(".", 1)[-1] in ("beta", "gamma")]
        assert len(scales) == 2 * len(R.block_prefixes(k, args)) and all(float(v.abs().min()) >= 0.5 for v in scales), name
        trivial = all(bool((sd[b] == (0.0 if b.endswith("mean") else 1.0)).all()) for b in R.buffers_of(k, args))
        assert trivial == training, name                          # eval cases run on seeded running statistics
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 512 * 1024, name
    assert R.CASES["sfh_stage_d4_n2"][1]["depth"] == 2 and R.CASES["sfh_stage_d4_n3_eval"][1]["depth"] == 3
    assert R.NET == dict(embed_dim=[4, 8, 16, 8, 4], depth=[1, 1, 2, 1, 1])
    assert len(R.BLOCK_PARAMS) == 40


def _module(N, kind, args):
    return {"block": N.Block, "stage": N.Stage, "net": N.Backbone}[kind](**args)


def test_modules_have_the_reference_keys_and_load_a_checkpoint():
    from image_restoration_amd import sfhformer as N
    import image_restoration_amd
    for name in ("Block", "Stage", "Backbone", "PatchEmbed", "PatchUnEmbed", "PatchUnEmbed_for_upsample", "DownSample", "SFHformer_t",
                 "SFHformer_s", "SFHformer_m", "SFHformer_l"):
        assert name in N.__all__ and hasattr(N, name)
    for name in ("SFHformer_t", "SFHformer_s", "SFHformer_m", "SFHformer_l"):
        assert getattr(image_restoration_amd, name) is getattr(N, name) and name in image_restoration_amd.__all__
    keys = load("sfh_block_keys")
    assert [t for t, _, _ in R.KEY_CASES] == ["block_d8", "stage_d6_n2", "net_tiny", "t"]
    for tag, kind, args in R.KEY_CASES:
        mod = N.SFHformer_t() if tag == "t" else _module(N, kind, args)
        sd = mod.state_dict()
        assert list(sd) == [str(k) for k in keys[tag + ".keys"]], tag
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys[tag + ".shapes"]], tag
        buffers = [k for k, _ in mod.named_buffers()]
        assert buffers == [str(k) for k in keys[tag + ".buffers"]] and len(buffers) == 9 * len(R.block_prefixes(kind, args)), tag
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.state_dict_layout(kind, args), tag
        assert [k for k, _ in mod.named_parameters()] == R.params_of(kind, args), tag
        state = R.module_state(kind, args, R.make_state(kind, args, 5, trivial_stats=False), steps=3)
        mod.load_state_dict(state, strict=True)
        assert all(torch.equal(mod.state_dict()[k], v) for k, v in state.items()), tag
    blk = N.Block(8)
    assert [k for k, _ in blk.named_parameters()] == list(R.BLOCK_PARAMS)
    assert [p.data_ptr() for p in N._block_params(blk)] == [p.data_ptr() for p in blk.parameters()]   # the order the op takes them in
    assert isinstance(blk.norm1, N.BatchNorm2d) and isinstance(blk.norm2, N.BatchNorm2d) and isinstance(blk.mixer, N.Mixer)
    assert isinstance(blk.ffn, N.FFN) and not blk.beta.detach().any() and not blk.gamma.detach().any()    # the reference's init
    assert [type(m) for m in N.Stage(3, 4).blocks] == [N.Block] * 3
    for name, depth in (("SFHformer_s", [2, 2, 4, 2, 2]), ("SFHformer_m", [4, 4, 8, 4, 4]), ("SFHformer_l", [6, 6, 10, 6, 6])):
        net = getattr(N, name)()
        assert [len(getattr(net, s).blocks) for s in R.STAGES] == depth and net.patch_embed.proj.out_channels == 32


def test_constructor_refusals():
    from image_restoration_amd import ops, sfhformer as N
    assert (ops.SFH_BLOCK_MAX_DIM, ops.SFH_BLOCK_MIN_HW, ops.SFH_BLOCK_MAX_HW, ops.SFH_BLOCK_PARAMS) == (128, 2, 512, 40)
    for bad in (5, 0, 130, 1, -2, 4.0):
        with pytest.raises(NotImplementedError, match="not covered"):
            N.Block(bad)
        with pytest.raises(NotImplementedError, match="not covered"):
            N.Stage(2, bad)
    with pytest.raises(NotImplementedError, match="defaults only"):
        N.Block(8, norm_layer=torch.nn.GroupNorm)
    with pytest.raises(NotImplementedError, match="defaults only"):
        N.Block(8, token_mixer=N.FFN)
    N.Block(8, norm_layer=torch.nn.BatchNorm2d), N.Block(8, norm_layer=N.BatchNorm2d, token_mixer=N.Mixer)
    for kw in (dict(patch_size=2), dict(patch_size=4, embed_kernel_size=4), dict(embed_kernel_size=1), dict(embed_kernel_size=5)):
        with pytest.raises(NotImplementedError, match="not covered"):
            N.Backbone(embed_dim=[4, 8, 16, 8, 4], depth=[1] * 5, **kw)
    with pytest.raises(NotImplementedError, match="not covered"):
        N.PatchEmbed(patch_size=4)
    with pytest.raises(NotImplementedError, match="not covered"):
        N.PatchUnEmbed(patch_size=1, kernel_size=None)
    with pytest.raises(NotImplementedError, match="not covered"):
        N.PatchUnEmbed_for_upsample(patch_size=4)
    with pytest.raises(ValueError, match="five entries"):
        N.Backbone(embed_dim=[4, 8, 16], depth=[1, 1, 1])
    with pytest.raises(ValueError, match="does not fit"):
        N.Backbone(embed_dim=[4, 8, 16, 8, 6], depth=[1] * 5)
    for mod in (N.Block(4), N.Stage(2, 4), N.Backbone(embed_dim=[4, 8, 16, 8, 4], depth=[1] * 5)):
        c = 3 if isinstance(mod, N.Backbone) else 4
        with pytest.raises(RuntimeError, match="MI355X only"):
            mod(torch.zeros(1, c, 8, 8))
    blk = N.Block(4)
    blk.norm2.momentum = 0.2
    with pytest.raises(NotImplementedError, match="share one eps"):       # the three norms of a Block must agree
        blk(torch.zeros(1, 4, 8, 8))
    blk = N.Block(4)
    blk.mixer.mixer_gloal.FFC.bn.eval()
    with pytest.raises(NotImplementedError, match="share one eps"):
        blk(torch.zeros(1, 4, 8, 8))
    blk = N.Block(4)
    blk.norm1.momentum = None
    with pytest.raises(NotImplementedError, match="fixed momentum"):
        blk(torch.zeros(1, 4, 8, 8))
    assert all(int(v) == 0 for k, v in blk.state_dict().items() if k.endswith("num_batches_tracked"))

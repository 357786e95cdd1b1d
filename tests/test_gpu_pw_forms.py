"""The 1x1 GEMM (csrc/pw_gemm.hip, csrc/pw_lds.hip) at every kernel instance, tile loop and descriptor feature.

The rows, the descriptor builder, the assertions and the CPU model live in tests/pw_forms.py; tests/test_cabi.py checks without a
GPU that the tables reach every instance and loop state.  Every case first asserts from ops.pw_plan of the descriptor it is about
to run that the call reaches the row's instance in the row's loop state (reach), then runs it on strided operands inside
NaN-guarded buffers.  Integer rows must equal the host result, rounded once to the output dtype, bit for bit - and so must the
kernel a row's switch replaces; LayerNorm rows are held to a bar built from a CPU model of the kernel's own roundings."""
import pytest
import torch

import pw_forms as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from image_restoration_amd import ops as o
    return o


def _launch(o, call):
    call.reset_outputs()
    o.pw_gemm_desc(call.d, DEV)
    call.check_guards()
    return call.result()


def _run_exact(monkeypatch, r):
    """reach, run, compare bit for bit with the host; then the same bits from the kernel the row's switches replace."""
    o = ops()
    P.set_switches(monkeypatch, r["env"])
    call = P.build(o, r, DEV)
    P.reach(o, r, call.d)
    got = _launch(o, call)
    assert torch.equal(got, call.ref), f"{P.case_id(r)}: max diff {float((got - call.ref).abs().max())} on {int((got != call.ref).sum())} elements"
    if r["replaced"]:
        P.set_switches(monkeypatch, r["replaced"])
        assert o.pw_plan(call.d)["family"] != r["key"][0], f"{P.case_id(r)}: {r['replaced']} does not replace the kernel"
        assert torch.equal(_launch(o, call), got), f"{P.case_id(r)}: the replaced kernel under {r['replaced']} gives other bits"
    return call, got


def _table(name):
    return pytest.mark.parametrize("r", P.TABLES[name], ids=P.case_id)


@_table("wave_loops")
def test_pw_wave_tile_loops(monkeypatch, r):
    """The tt loop of the X-resident and the streaming wave forms at 2 and 3 pixel tiles per wave on 19 tiles: the next-tile
    prefetch, a range that ends inside the plane, a second tile past it, idle waves; both store paths; bf16 and fp8 operands."""
    _run_exact(monkeypatch, r)


@_table("xcd")
def test_pw_xcd_map_is_a_permutation(monkeypatch, r):
    """The workgroup permutation of the streaming form: the same bits as the plain order."""
    call, got = _run_exact(monkeypatch, r)
    P.set_switches(monkeypatch, {})
    assert not ops().pw_plan(call.d)["xcd_map"]
    assert torch.equal(_launch(ops(), call), got)


@_table("resident")
def test_pw_resident_tile_loop_and_partial_tiles(monkeypatch, r):
    """The weight-resident kernel: several pixel tiles per workgroup with a ragged last workgroup, a partial pixel tile under the
    default switches, every tile height, and the K at which it hands over to the chunked kernel."""
    _run_exact(monkeypatch, r)


@_table("xwide")
def test_pw_xwide_slab_pipeline(monkeypatch, r):
    """The X-wide form's double-buffered weight slabs: one slab per workgroup, 2 of 5 with a ragged last workgroup, all 5 (odd
    count, both buffer parities); every K-chunk count, per-image weights, a panel seam inside a 32-k chunk."""
    _run_exact(monkeypatch, r)


@_table("chunked")
def test_pw_chunked_every_tile_height(monkeypatch, r):
    """The chunked kernel at every tile height of both dtypes: a plane of 35 pixels (scalar loads), an aligned one, and aligned
    rows behind a pointer one element off."""
    _run_exact(monkeypatch, r)


@_table("dma")
def test_pw_lds_dma_ring(monkeypatch, r):
    _run_exact(monkeypatch, r)


@_table("lds")
def test_pw_lds_tiled_exact_on_integers(monkeypatch, r):
    """The LDS-tiled deep-K family at both tile heights, a ragged M, a K tail inside a 64-k chunk and a partial 256-pixel tile."""
    _run_exact(monkeypatch, r)


@_table("split")
def test_pw_split_output(monkeypatch, r):
    """y_split on a row, inside a fragment, on a tile seam and on the last row; y2 has strides and a NaN guard of its own."""
    _run_exact(monkeypatch, r)


@_table("weights")
def test_pw_per_image_weight_sources(monkeypatch, r):
    """Own pack, bf16 copy and direct fp32 staging of per-image weights on each wave family.  The fp32 matrix holds other values
    than the copy, so the result shows which one the kernel read: the copy where the plan says b16, the matrix elsewhere."""
    _run_exact(monkeypatch, r)


@_table("f8")
def test_pw_fp8_instances_exact_on_integers(monkeypatch, r):
    """Every fp8 instance at unit scales: e4m3 holds the small integers exactly, so the result equals the integer reference."""
    _run_exact(monkeypatch, r)


@_table("ln")
def test_pw_layernorm_on_load(monkeypatch, r):
    """LayerNorm on load at its four instances, both modes, with and without the statistics, inside the xres tile loop.
    e = max|. - R| / max|R| against the fp64 statement R; the kernel may be no further off than 1.5 x the CPU model of its own
    roundings plus one bf16 ulp at the largest magnitude."""
    o = ops()
    P.set_switches(monkeypatch, r["env"])
    call = P.build(o, r, DEV)
    P.reach(o, r, call.d)
    got = _launch(o, call)
    ref, mu, rstd = P.ln_model(call.host, r["ln"], "fp64")
    model, _, _ = P.ln_model(call.host, r["ln"], "kernel", f8=r["f8"])
    e_model, e_gpu = P.rel_err(model, ref), P.rel_err(got, ref)
    print(f"{P.case_id(r)}: e_gpu {e_gpu:.3e} e_model {e_model:.3e} ratio {e_gpu / e_model:.3f}")
    # first run on an MI355X: e_gpu / e_model = 1.000 on all 33 rows (e 2.8e-3 .. 4.3e-3 on the bf16 rows, 3.7e-2 on the fp8 row):
    # the worst element carries the model's own roundings
    assert e_gpu <= P.ln_bar(e_model), f"{P.case_id(r)}: e_gpu {e_gpu:.3e} over the bar {P.ln_bar(e_model):.3e} (e_model {e_model:.3e})"
    if r["stats"]:
        for name, want in (("ln_mean", mu), ("ln_rstd", rstd)):
            e = P.rel_err(call.views[name].float().cpu(), want)
            assert e < P.BAR_STATS, f"{P.case_id(r)}: {name} off fp64 by {e:.3e}"

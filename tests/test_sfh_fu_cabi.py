"""Host-only checks of the FourierUnit entry points: the symbols and their signatures, mi_fourier_unit_plan against the two sizing
calls over a sweep of shapes, every refusal (no device is touched), the byte condition behind "the grouped conv's output is never
materialised", and the CPU-tensor refusal."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from plan_checks import sections_tile  # noqa: E402

SYMBOLS = ("mi_fourier_unit_workspace", "mi_fourier_unit_saved_bytes", "mi_fourier_unit_plan", "mi_fourier_unit_fwd",
           "mi_fourier_unit_bwd")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


def _exported(path):
    """Names the shared library defines in its dynamic symbol table (ELF64 little endian, read here: no binutils needed)."""
    import struct
    blob = open(path, "rb").read()
    assert blob[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, typ, _, _, off, size, link, _, _, entsize in secs:
        if typ != 11:                                  # SHT_DYNSYM
            continue
        stroff = secs[link][4]
        for k in range(size // entsize):
            name, _, _, shndx = struct.unpack_from("<IBBH", blob, off + k * entsize)
            if shndx != 0:
                names.add(blob[stroff + name:blob.index(b"\0", stroff + name)].decode())
    return names


def test_symbols_exist_with_their_signatures(lib):
    handle = lib.lib()
    header = open(os.path.join(ROOT, "include", "mi_restore.h")).read()
    declared = set(re.findall(r"\b(mi_fourier_unit_\w+)\(", header))
    dynsym = _exported(lib.LIB_PATH)
    assert "mi_version" in dynsym and "mi_dft2_r2c" in dynsym
    exported = {n for n in dynsym if n.startswith("mi_fourier_unit_")}
    table = {k for k in lib.SIGNATURES if k.startswith("mi_fourier_unit_")}
    assert declared == exported == table == set(SYMBOLS)
    for name in SYMBOLS:
        fn = getattr(handle, name)
        res, args = lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert C.sizeof(lib.FourierUnitShape) == 7 * C.sizeof(C.c_int) + 2 * C.sizeof(C.c_float)
    assert C.sizeof(lib.FourierUnitParams) == 8 * C.sizeof(C.c_void_p)
    assert C.sizeof(lib.FourierUnitGrads) == 9 * C.sizeof(C.c_void_p)      # eight pointers, the flag, padding
    # shape, parameters, x, out, the two running statistics, saved, ws, stream / shape, parameters, dout, dx, gradients, saved, ws, stream
    assert len(lib.SIGNATURES["mi_fourier_unit_fwd"][1]) == 9 and len(lib.SIGNATURES["mi_fourier_unit_bwd"][1]) == 8
    # the transform launchers shared with FreMLP stay internal
    internal = ("dft2_r2c_run", "dft2_tables", "dft2_c2r_adj", "dft2_geom", "dft2_blob", "dft2_rows_fwd", "dft2_cols")
    assert not any(name in n for name in internal for n in dynsym)


# B, c, groups, H, W
SWEEP = [(1, 1, 1, 2, 2), (1, 1, 2, 2, 2), (2, 6, 4, 5, 7), (2, 8, 4, 8, 12), (1, 4, 1, 4, 4), (2, 4, 2, 6, 10), (3, 10, 4, 100, 130),
         (1, 256, 4, 4, 6), (1, 256, 8, 8, 8), (2, 8, 4, 16, 16), (1, 3, 6, 512, 512), (8, 64, 4, 256, 256), (8, 128, 4, 128, 128),
         (8, 256, 4, 64, 64), (5, 7, 7, 33, 65), (2, 12, 3, 9, 16)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_plan_is_consistent_with_the_sizing_calls(lib, dtype):
    from image_restoration_amd import ops
    for B, c, G, H, W in SWEEP:
        p = ops.fourier_unit_plan(B, c, G, H, W, dtype)
        saved, ws = ops.fourier_unit_sizes(B, c, G, H, W, dtype)
        assert (p["saved_bytes"], p["workspace"]) == (saved, ws) and saved > 0 and ws > 0
        K, C2 = W // 2 + 1, 2 * c
        N = H * K
        elems = B * C2 * N
        assert (p["planes"], p["K"], p["channels"], p["groups"], p["group_width"]) == (B * c, K, C2, G, C2 // G)
        assert (p["elements"], p["bins"], p["block"]) == (elems, B * N, 256)
        assert p["chunks_per_plane"] == -(-N // p["bn_chunk"]) and p["partials_per_channel"] == B * p["chunks_per_plane"]
        assert p["grid_elements"] == B * C2 * -(-N // 1024) and p["grid_bins"] == -(-B * N // 64)
        assert (p["kernels_fwd"], p["kernels_bwd"], p["lib_calls_fwd"], p["lib_calls_bwd"]) == (11, 14, 1, 6)
        # the blob: Z (two floats per bin and channel), then (mu, r) per spectral channel; nothing else
        assert p["saved_stat_offset"] >= 4 * elems and saved >= p["saved_stat_offset"] + 8 * C2 and saved < 4 * elems + 8 * C2 + 512
        sec = p["sections"]
        assert sections_tile(sec)[0] <= ws
        # the transforms' blob: its tables, then its one complex intermediate, contiguous
        assert sec["dft_T"][0] == sec["dft_tables"][0] + sec["dft_tables"][1]
        assert sec["Z"][0] - sec["dft_tables"][0] == lib.lib().mi_dft2_workspace(B, c, H, W)
        for name in ("dft_T", "Z", "U", "t", "ts", "pre", "q"):
            assert sec[name][1] == 4 * elems, name
        assert sec["s"][1] == sec["dlogit"][1] == 4 * B * G * N
        assert sec["stat"][1] == 16 * C2 and sec["w_fold"][1] == 4 * C2 * C2 and sec["grad_tmp"][1] == 4 * (C2 * C2 + 2 * G * C2)
        assert sec["bn_partials"][1] == 8 * C2 * p["partials_per_channel"] and sec["bwd_partials"][1] == 48 * C2 * p["partials_per_channel"]
    assert ops.fourier_unit_sizes(2, 6, 4, 5, 7, torch.float32) == ops.fourier_unit_sizes(2, 6, 4, 5, 7, torch.bfloat16)


def test_the_grouped_conv_output_is_never_materialised(lib):
    """A plan condition, not a measurement: at c = 64, G = 4, B = 8, 256 x 256 no workspace or saved section exceeds one complex fp32
    spectrum, 8 B c H K bytes; the grouped conv's [B, G 2c, H, K] output would be four times that."""
    from image_restoration_amd import ops
    B, c, G, H, W = 8, 64, 4, 256, 256
    spectrum = 8 * B * c * H * (W // 2 + 1)
    for dtype in (torch.float32, torch.bfloat16):
        p = ops.fourier_unit_plan(B, c, G, H, W, dtype)
        for name, (_, nbytes) in p["sections"].items():
            assert nbytes <= spectrum, (name, nbytes, spectrum)
        assert p["saved_stat_offset"] == spectrum and p["saved_bytes"] - p["saved_stat_offset"] <= 8 * 2 * c + 256
        assert max(n for _, n in p["sections"].values()) == spectrum


def test_every_refusal_returns_before_a_launch(lib):
    """No device exists in this test: a call that tried to launch would fail differently (or crash on the null pointers)."""
    L, handle = lib, lib.lib()
    out = (L.c_i64 * 64)()

    def shape(B=2, c=8, groups=4, H=8, W=8, dtype=0, training=1, eps=1e-5, momentum=0.1):
        return L.FourierUnitShape(B, c, groups, H, W, dtype, training, eps, momentum)

    assert handle.mi_fourier_unit_plan(C.byref(shape()), out) == 0
    assert handle.mi_fourier_unit_plan(C.byref(shape(c=6)), out) == 0            # c % G != 0 with 2c % G == 0
    assert handle.mi_fourier_unit_plan(C.byref(shape(c=256, groups=8, H=2, W=2)), out) == 0
    bad = [(dict(c=5, groups=4), b"no multiple"), (dict(groups=9, c=9), b"groups=9"), (dict(groups=0), b"groups=0"),
           (dict(c=257, groups=2), b"c=257"), (dict(c=0), b"c=0"), (dict(H=1), b"H=1"), (dict(W=1), b"W=1"), (dict(H=513), b"H=513"),
           (dict(W=513), b"W=513"), (dict(dtype=7), b"bad dtype 7"), (dict(B=0), b"B=0"), (dict(eps=0.0), b"eps"),
           (dict(momentum=1.5), b"momentum"), (dict(B=300, c=256, H=512, W=512), b"too many bins")]
    pp, gg = L.FourierUnitParams(), L.FourierUnitGrads()
    for kw, msg in bad:
        s = shape(**kw)
        assert handle.mi_fourier_unit_plan(C.byref(s), out) != 0, kw
        assert msg in handle.mi_last_error(), (kw, handle.mi_last_error())
        assert handle.mi_fourier_unit_workspace(C.byref(s)) == 0 and handle.mi_fourier_unit_saved_bytes(C.byref(s)) == 0
        p = C.cast(256, C.c_void_p)        # never dereferenced: the shape is refused first
        fp = C.cast(256, C.POINTER(C.c_float))
        assert handle.mi_fourier_unit_fwd(C.byref(s), C.byref(pp), p, p, fp, fp, p, p, None) != 0, kw
        assert handle.mi_fourier_unit_bwd(C.byref(s), C.byref(pp), p, p, C.byref(gg), p, p, None) != 0, kw
    assert handle.mi_fourier_unit_plan(None, out) != 0 and b"null shape" in handle.mi_last_error()
    assert handle.mi_fourier_unit_plan(C.byref(shape()), None) != 0
    assert handle.mi_fourier_unit_workspace(None) == 0 and handle.mi_fourier_unit_saved_bytes(None) == 0
    # null tensors with a good shape
    assert handle.mi_fourier_unit_fwd(C.byref(shape()), C.byref(pp), None, None, None, None, None, None, None) != 0
    assert b"null" in handle.mi_last_error()
    assert handle.mi_fourier_unit_bwd(C.byref(shape()), C.byref(pp), None, None, C.byref(gg), None, None, None) != 0
    assert b"null" in handle.mi_last_error()
    assert handle.mi_fourier_unit_fwd(C.byref(shape()), None, None, None, None, None, None, None, None) != 0


def test_module_refuses_what_the_kernels_do_not_cover_and_cpu_tensors(lib):
    from image_restoration_amd import ops, sfhformer as N
    with pytest.raises(NotImplementedError, match="in_channels == out_channels"):
        N.FourierUnit(8, 16)
    for bad in (dict(in_channels=5, out_channels=5, groups=4), dict(in_channels=9, out_channels=9, groups=9),
                dict(in_channels=257, out_channels=257, groups=2), dict(in_channels=0, out_channels=0)):
        with pytest.raises(NotImplementedError, match="not covered"):
            N.FourierUnit(**bad)
    N.FourierUnit(256, 256, 8), N.FourierUnit(6, 6), N.FourierUnit(1, 1, 1)
    mod = N.FourierUnit(8, 8)
    with pytest.raises(RuntimeError, match="MI355X only"):
        mod(torch.zeros(1, 8, 8, 8))
    assert int(mod.bn.num_batches_tracked) == 0          # a refused call counts no batch
    params = [mod.bn.weight, mod.bn.bias, mod.fdc.weight, mod.fdc.bias, mod.weight[0].weight, mod.weight[0].bias, mod.fpe.weight,
              mod.fpe.bias]
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.fourier_unit_fwd(torch.zeros(1, 8, 8, 8), params, mod.bn.running_mean, mod.bn.running_var, True, False)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.fourier_unit_bwd(torch.zeros(1, 8, 8, 8), params, torch.zeros(8), [torch.zeros_like(p) for p in params], False, True)
    mod.bn.momentum = None
    with pytest.raises(NotImplementedError, match="fixed momentum"):
        mod(torch.zeros(1, 8, 8, 8))

"""Drop-in replacements for the reference's ``DRSformer_arch.py``: its transformer blocks, its MEFC and the whole network.

``Attention`` (TKSA, top-k sparse attention, :101-171), ``FeedForward`` (MSFN, mixed-scale FFN, :62-98) and
``TransformerBlock`` (STB, :174-187) keep the reference's class names, constructor arguments, parameter names and shapes
(``state_dict`` interchangeable) and ``forward`` signatures; ``forward`` runs the gfx950 kernels through the C-ABI
(``mi_tksa_*``, ``mi_msfn_*``, ``mi_ln_*``).  The conv submodules are parameter containers only.  Activations may be float32
(the parity path) or bfloat16; parameters and their gradients stay float32.  ``main_grad`` accumulation (FlatTrainer) as in
:mod:`image_restoration_amd.restormer`.  CPU tensors are refused: there is no fallback.

The top-k sizes are computed here with the reference's own expressions (``ops.tksa_topk``) and handed to the kernels; the
masks are ranked on the device from the fp32 scores, so nothing syncs with the host and the modules capture into HIP graphs.
``Attention.record_scores = True`` keeps the last forward's scores (``Attention.scores``, [B, heads, c, c] fp32): the S the
masks were ranked from, for tests and inspection.  Likewise ``FeedForward.record_masks = True`` keeps the last training
forward's ReLU decisions (``FeedForward.relu_masks``: a > 0, b > 0, y > 0 of the saved planes, [B, 2h, H, W] bool).

The Mixture of Experts Feature Compensator (``subnet``, :328-354, with ``OALayer``, ``GroupOLs``, ``OperationLayer``,
``SepConv``, ``DilConv``) runs one layer pair (routing head + GroupOLs) as one autograd node on ``mi_mefc_*``; its submodules are
parameter containers whose own ``forward`` raises (the pair is computed whole).  ``subnet.record_masks = True`` keeps the last
training forward's ReLU decisions and routing weights (``subnet.relu_masks``: one dict per layer pair, see ``_mefc_record``).
``DRSformer`` (:388-480) assembles the U-Net from these, the STB and Restormer's native glue (patch embed, resampling, the
concat-free ``reduce_chan`` 1x1s, the output conv with its ``+ inp_img`` residual).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._autograd import module_op
from .restormer import Downsample, LayerNorm, OverlapPatchEmbed, Upsample, _conv1x1_module, _conv2d, _stage, _up_cat

Tensor = torch.Tensor

__all__ = ["Attention", "FeedForward", "TransformerBlock", "LayerNorm", "SepConv", "DilConv", "OperationLayer", "GroupOLs",
           "OALayer", "subnet", "OverlapPatchEmbed", "Downsample", "Upsample", "DRSformer", "Operations"]


def _scores_to(owner, scores) -> None:
    if scores is not None:
        owner.scores = scores


def _relu_masks_to(ffn, x, saved) -> None:
    if ffn.record_masks and saved is not None:
        v = ops.msfn_saved_views(saved, x, ffn.dwconv3x3_1.weight.shape[0])
        ffn.relu_masks = (v["a"] > 0, v["b"] > 0, v["y"] > 0)


class _TksaOp:
    """Attention.forward (TKSA).  params: ops.tksa_fwd; saved = [the kernels' blob].  ``dim``: the channel count of x."""

    def __init__(self, owner, dim):
        self.owner, self.heads, self.topk = owner, owner.num_heads, owner.topk(dim)

    def fwd(self, x, residual, params, need):
        """-> (out, blob); keeps the scores on the owner when it records them."""
        res = ops.tksa_fwd(x, residual, params, self.heads, self.topk, need, want_scores=self.owner.record_scores)
        _scores_to(self.owner, res[2] if self.owner.record_scores else None)
        return res[0], res[1]

    def forward(self, acts, params, need):
        out, blob = self.fwd(acts[0], None, params, need)
        return out, [blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.tksa_bwd(acts[0], dout, params, self.heads, self.topk, saved[0], grads, acc),)


class _MsfnOp:
    """FeedForward.forward (MSFN).  params: ops.msfn_fwd; saved = [the kernels' blob]."""

    def __init__(self, owner):
        self.owner = owner

    def fwd(self, x, residual, params, need):
        """-> (out, blob); keeps the ReLU decisions on the owner when it records them."""
        out, blob = ops.msfn_fwd(x, residual, params, need)
        _relu_masks_to(self.owner, x, blob)
        return out, blob

    def forward(self, acts, params, need):
        out, blob = self.fwd(acts[0], None, params, need)
        return out, [blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.msfn_bwd(acts[0], dout, params, saved[0], grads, acc),)


def split_block(params):
    """The STB's parameter (and gradient) layout: norm1 (2), TKSA (11), norm2 (2), MSFN (12)."""
    return params[0:2], params[2:13], params[13:15], params[15:27]


class _StbOp:
    """x + attn(norm1(x)), then + ffn(norm2(.)) (DRSformer_arch.py:183-187) as one module op; both residual adds run in
    the epilogue of the producing 1x1 GEMM, and their gradients enter the LayerNorm backward kernels (dres).
    saved = [xn, y, yn, mean1, rstd1, mean2, rstd2, sv_a, sv_f]."""

    def __init__(self, owner, dim):
        self.attn, self.ffn = _TksaOp(owner.attn, dim), _MsfnOp(owner.ffn)

    def forward(self, acts, params, need):
        x = acts[0]
        n1, att, n2, ffn = split_block(params)
        wb = n1[1] is not None
        xn, mean1, rstd1 = ops.ln_fwd(x, n1[0], n1[1], wb, want_stats=need)
        y, sv_a = self.attn.fwd(xn, x, att, need)
        yn, mean2, rstd2 = ops.ln_fwd(y, n2[0], n2[1], wb, want_stats=need)
        out, sv_f = self.ffn.fwd(yn, y, ffn, need)
        return out, [xn, y, yn, mean1, rstd1, mean2, rstd2, sv_a, sv_f]

    def backward(self, acts, saved, dout, params, grads, acc):
        xn, y, yn, mean1, rstd1, mean2, rstd2, sv_a, sv_f = saved
        n1, att, n2, ffn = split_block(params)
        g1, ga, g2, gf = split_block(grads)
        wb = n1[1] is not None
        dyn, = self.ffn.backward((yn,), (sv_f,), dout, ffn, gf, acc)
        dy = ops.ln_bwd(dyn, y, n2[0], mean2, rstd2, dout, wb, g2[0], g2[1], acc)
        dxn, = self.attn.backward((xn,), (sv_a,), dy, att, ga, acc)
        return (ops.ln_bwd(dxn, acts[0], n1[0], mean1, rstd1, dy, wb, g1[0], g1[1], acc),)


class FeedForward(nn.Module):
    """MSFN (DRSformer_arch.py:62-98)."""

    def __init__(self, dim, ffn_expansion_factor, bias):
        super().__init__()
        hidden_features = int(dim * ffn_expansion_factor)
        h2 = hidden_features * 2
        self.project_in = nn.Conv2d(dim, h2, kernel_size=1, bias=bias)
        self.dwconv3x3 = nn.Conv2d(h2, h2, kernel_size=3, stride=1, padding=1, groups=h2, bias=bias)
        self.dwconv5x5 = nn.Conv2d(h2, h2, kernel_size=5, stride=1, padding=2, groups=h2, bias=bias)
        self.relu3 = nn.ReLU()
        self.relu5 = nn.ReLU()
        self.dwconv3x3_1 = nn.Conv2d(h2, hidden_features, kernel_size=3, stride=1, padding=1, groups=hidden_features, bias=bias)
        self.dwconv5x5_1 = nn.Conv2d(h2, hidden_features, kernel_size=5, stride=1, padding=2, groups=hidden_features, bias=bias)
        self.relu3_1 = nn.ReLU()
        self.relu5_1 = nn.ReLU()
        self.project_out = nn.Conv2d(h2, dim, kernel_size=1, bias=bias)
        self.record_masks = False
        self.relu_masks = None

    def _params(self):
        return (self.project_in.weight, self.project_in.bias, self.dwconv3x3.weight, self.dwconv3x3.bias,
                self.dwconv5x5.weight, self.dwconv5x5.bias, self.dwconv3x3_1.weight, self.dwconv3x3_1.bias,
                self.dwconv5x5_1.weight, self.dwconv5x5_1.bias, self.project_out.weight, self.project_out.bias)

    def forward(self, x):
        return module_op(_MsfnOp(self), (x,), self._params())


class Attention(nn.Module):
    """TKSA (DRSformer_arch.py:101-171)."""

    def __init__(self, dim, num_heads, bias):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Conv2d(dim, dim * 3, kernel_size=1, bias=bias)
        self.qkv_dwconv = nn.Conv2d(dim * 3, dim * 3, kernel_size=3, stride=1, padding=1, groups=dim * 3, bias=bias)
        self.project_out = nn.Conv2d(dim, dim, kernel_size=1, bias=bias)
        self.attn_drop = nn.Dropout(0.)
        self.attn1 = nn.Parameter(torch.tensor([0.2]), requires_grad=True)
        self.attn2 = nn.Parameter(torch.tensor([0.2]), requires_grad=True)
        self.attn3 = nn.Parameter(torch.tensor([0.2]), requires_grad=True)
        self.attn4 = nn.Parameter(torch.tensor([0.2]), requires_grad=True)
        self.record_scores = False
        self.scores = None

    def topk(self, dim: int):
        return ops.tksa_topk(dim // self.num_heads)

    def _params(self):
        return (self.temperature, self.qkv.weight, self.qkv.bias, self.qkv_dwconv.weight, self.qkv_dwconv.bias,
                self.project_out.weight, self.project_out.bias, self.attn1, self.attn2, self.attn3, self.attn4)

    def forward(self, x):
        return module_op(_TksaOp(self, x.shape[1]), (x,), self._params())


class TransformerBlock(nn.Module):
    """Sparse Transformer Block: norm1 -> attn -> +x -> norm2 -> ffn -> +x (DRSformer_arch.py:174-187), one autograd node."""

    def __init__(self, dim, num_heads, ffn_expansion_factor, bias, LayerNorm_type):
        super().__init__()
        self.norm1 = LayerNorm(dim, LayerNorm_type)
        self.attn = Attention(dim, num_heads, bias)
        self.norm2 = LayerNorm(dim, LayerNorm_type)
        self.ffn = FeedForward(dim, ffn_expansion_factor, bias)

    def forward(self, x):
        params = self.norm1._params() + self.attn._params() + self.norm2._params() + self.ffn._params()
        return module_op(_StbOp(self, x.shape[1]), (x,), params)


# ====================================================================================== MEFC (DRSformer_arch.py:189-354)
Operations = ['sep_conv_1x1', 'sep_conv_3x3', 'sep_conv_5x5', 'sep_conv_7x7', 'dil_conv_3x3', 'dil_conv_5x5', 'dil_conv_7x7',
              'avg_pool_3x3']


def _whole_pair_only(name):
    raise NotImplementedError(f"image_restoration_amd: {name} runs inside subnet only (one mi_mefc_* call per OALayer + GroupOLs "
                              "pair); its modules hold the parameters")


class SepConv(nn.Module):
    """dw k x k -> 1x1 -> ReLU -> dw k x k -> 1x1 (:284-296); parameter container."""

    def __init__(self, C_in, C_out, kernel_size, stride, padding, affine=True):
        super().__init__()
        self.op = nn.Sequential(
            nn.Conv2d(C_in, C_in, kernel_size=kernel_size, stride=stride, padding=padding, groups=C_in, bias=False),
            nn.Conv2d(C_in, C_in, kernel_size=1, padding=0, bias=False),
            nn.ReLU(inplace=False),
            nn.Conv2d(C_in, C_in, kernel_size=kernel_size, stride=1, padding=padding, groups=C_in, bias=False),
            nn.Conv2d(C_in, C_out, kernel_size=1, padding=0, bias=False),)

    def forward(self, x):
        _whole_pair_only("SepConv")


class DilConv(nn.Module):
    """dw k x k with dilation -> 1x1 (:259-267); parameter container."""

    def __init__(self, C_in, C_out, kernel_size, stride, padding, dilation, affine=True):
        super().__init__()
        self.op = nn.Sequential(
            nn.Conv2d(C_in, C_in, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, groups=C_in,
                      bias=False),
            nn.Conv2d(C_in, C_out, kernel_size=1, padding=0, bias=False),)

    def forward(self, x):
        _whole_pair_only("DilConv")


class ReLUConv(nn.Module):
    """1x1 conv -> ReLU (:250-257): GroupOLs.preprocess."""

    def __init__(self, C_in, C_out, kernel_size, stride, padding, affine=True):
        super().__init__()
        self.op = nn.Sequential(nn.Conv2d(C_in, C_out, kernel_size, stride=stride, padding=padding, bias=False),
                                nn.ReLU(inplace=False))

    def forward(self, x):
        _whole_pair_only("ReLUConv")


def _op(name, C, stride):
    k = int(name[-1])
    if name.startswith("sep"):
        return SepConv(C, C, k, stride, k // 2, affine=False)
    if name.startswith("dil"):
        return DilConv(C, C, k, stride, k - 1, 2, affine=False)
    return nn.AvgPool2d(3, stride=stride, padding=1, count_include_pad=False)


class OperationLayer(nn.Module):
    """The eight weighted operations and the 8C -> C projection (:189-204)."""

    def __init__(self, C, stride):
        super().__init__()
        if stride != 1:
            raise NotImplementedError("image_restoration_amd: OperationLayer is built for stride 1 (DRSformer's only use)")
        self._ops = nn.ModuleList([_op(o, C, stride) for o in Operations])
        self._out = nn.Sequential(nn.Conv2d(C * len(Operations), C, 1, padding=0, bias=False), nn.ReLU())

    def _params(self):
        ps = []
        for i in range(4):
            s = self._ops[i].op
            ps += [s[0].weight, s[1].weight, s[3].weight, s[4].weight]
        for i in range(4, 7):
            d = self._ops[i].op
            ps += [d[0].weight, d[1].weight]
        return ps + [self._out[0].weight]

    def forward(self, x, weights):
        _whole_pair_only("OperationLayer")


class GroupOLs(nn.Module):
    """preprocess, then ``steps`` residual OperationLayers (:206-225)."""

    def __init__(self, steps, C):
        super().__init__()
        self.preprocess = ReLUConv(C, C, 1, 1, 0, affine=False)
        self._steps = steps
        self._ops = nn.ModuleList([OperationLayer(C, 1) for _ in range(steps)])
        self.relu = nn.ReLU()

    def forward(self, s0, weights):
        _whole_pair_only("GroupOLs")


class OALayer(nn.Module):
    """Routing head: global average pool, Linear -> ReLU -> Linear, viewed [B, k, num_ops] (:227-247)."""

    def __init__(self, channel, k, num_ops):
        super().__init__()
        self.k = k
        self.num_ops = num_ops
        self.output = k * num_ops
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.ca_fc = nn.Sequential(nn.Linear(channel, self.output * 2), nn.ReLU(), nn.Linear(self.output * 2, self.k * self.num_ops))

    def forward(self, x):
        _whole_pair_only("OALayer")


def _mefc_record(owner, x, saved, out, steps) -> None:
    """ReLU decisions and routing weights of one training forward of a layer pair: pre0 (preprocess, s_0 > 0), h (routing hidden
    layer), per step u (pw1 outputs U > 0, [B, 4C, H, W]), pre (out projection > 0) and out (residual ReLU: s_{t+1} > 0), and w
    ([B, steps, 8] fp32)."""
    v = ops.mefc_saved_views(saved, x, steps)
    s_next = v["s"][1:] + [out]
    owner.relu_masks.append({"pre0": v["s"][0] > 0, "h": v["hpre"] > 0, "u": [u > 0 for u in v["u"]],
                             "pre": [p > 0 for p in v["pre"]], "out": [s > 0 for s in s_next], "w": v["w"].clone()})


class _MefcOp:
    """One OALayer + GroupOLs pair (DRSformer_arch.py:346-351) as one module op.  params: ops.mefc_fwd; saved = [out (the
    backward reads the pair's own output), the kernels' blob]."""

    def __init__(self, owner, steps):
        self.owner, self.steps = owner, steps

    def forward(self, acts, params, need):
        out, blob = ops.mefc_fwd(acts[0], params, self.steps, need)
        if self.owner.record_masks and blob is not None:
            _mefc_record(self.owner, acts[0], blob, out, self.steps)
        return out, [out, blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.mefc_bwd(acts[0], saved[0], dout, params, self.steps, saved[1], grads, acc),)


class subnet(nn.Module):  # noqa: N801  (the reference's class name)
    """Mixture of Experts Feature Compensator (:328-354): ``layer_num`` pairs of (OALayer, GroupOLs)."""

    def __init__(self, dim, layer_num=1, steps=4):
        super().__init__()
        self._C = dim
        self.num_ops = len(Operations)
        self._layer_num = layer_num
        self._steps = steps
        self.layers = nn.ModuleList()
        for _ in range(self._layer_num):
            self.layers += [OALayer(self._C, self._steps, self.num_ops)]
            self.layers += [GroupOLs(steps, self._C)]
        self.record_masks = False
        self.relu_masks = None

    def pair_params(self, i):
        oal, grp = self.layers[2 * i], self.layers[2 * i + 1]
        ps = [oal.ca_fc[0].weight, oal.ca_fc[0].bias, oal.ca_fc[2].weight, oal.ca_fc[2].bias, grp.preprocess.op[0].weight]
        for op in grp._ops:
            ps += op._params()
        return ps

    def forward(self, x):
        ops._gpu(x)
        if self.record_masks and torch.is_grad_enabled():
            self.relu_masks = []
        x = x.contiguous()
        for i in range(self._layer_num):
            x = module_op(_MefcOp(self, self._steps), (x,), self.pair_params(i))
        return x


# ====================================================================================== the network (DRSformer_arch.py:388-480)
class DRSformer(nn.Module):
    """The reference U-Net over the native STB and MEFC; same constructor and state_dict."""

    def __init__(self, inp_channels=3, out_channels=3, dim=48, num_blocks=[4, 6, 6, 8], heads=[1, 2, 4, 8],
                 ffn_expansion_factor=2.66, bias=False, LayerNorm_type='WithBias'):
        super().__init__()

        def stage(c, h, n):
            return _stage(c, h, n, ffn_expansion_factor, bias, LayerNorm_type, block=TransformerBlock)

        self.patch_embed = OverlapPatchEmbed(inp_channels, dim)
        self.encoder_level0 = subnet(dim)
        self.encoder_level1 = stage(dim, heads[0], num_blocks[0])
        self.down1_2 = Downsample(dim)
        self.encoder_level2 = stage(int(dim * 2 ** 1), heads[1], num_blocks[1])
        self.down2_3 = Downsample(int(dim * 2 ** 1))
        self.encoder_level3 = stage(int(dim * 2 ** 2), heads[2], num_blocks[2])
        self.down3_4 = Downsample(int(dim * 2 ** 2))
        self.latent = stage(int(dim * 2 ** 3), heads[3], num_blocks[3])
        self.up4_3 = Upsample(int(dim * 2 ** 3))
        self.reduce_chan_level3 = nn.Conv2d(int(dim * 2 ** 3), int(dim * 2 ** 2), kernel_size=1, bias=bias)
        self.decoder_level3 = stage(int(dim * 2 ** 2), heads[2], num_blocks[2])
        self.up3_2 = Upsample(int(dim * 2 ** 2))
        self.reduce_chan_level2 = nn.Conv2d(int(dim * 2 ** 2), int(dim * 2 ** 1), kernel_size=1, bias=bias)
        self.decoder_level2 = stage(int(dim * 2 ** 1), heads[1], num_blocks[1])
        self.up2_1 = Upsample(int(dim * 2 ** 1))
        self.decoder_level1 = stage(int(dim * 2 ** 1), heads[0], num_blocks[0])
        self.refinement = subnet(dim=int(dim * 2 ** 1))
        self.output = nn.Conv2d(int(dim * 2 ** 1), out_channels, kernel_size=3, stride=1, padding=1, bias=bias)

    def forward(self, inp_img):
        inp_enc_level1 = self.patch_embed(inp_img)
        out_enc_level1 = self.encoder_level1(self.encoder_level0(inp_enc_level1))
        out_enc_level2 = self.encoder_level2(self.down1_2(out_enc_level1))
        out_enc_level3 = self.encoder_level3(self.down2_3(out_enc_level2))
        latent = self.latent(self.down3_4(out_enc_level3))
        # concat-free channel reduce: two K-panels of one 1x1 GEMM (:467-473); level 1 concatenates without one (:475-477)
        out_dec_level3 = self.decoder_level3(_conv1x1_module(self.up4_3(latent), out_enc_level3, self.reduce_chan_level3))
        out_dec_level2 = self.decoder_level2(_conv1x1_module(self.up3_2(out_dec_level3), out_enc_level2, self.reduce_chan_level2))
        out_dec_level1 = self.decoder_level1(_up_cat(self.up2_1, out_dec_level2, out_enc_level1))
        out_dec_level1 = self.refinement(out_dec_level1)
        return _conv2d(out_dec_level1, self.output, inp_img)

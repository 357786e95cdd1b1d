"""World-size-2 gloo test of gradient-norm clipping and the weight EMA of FlatTrainer (max_grad_norm / ema_decay): with the
all-reduce overlapped with backward, after backward, and with the sharded optimizer, both ranks must report the norm of the MEAN
gradient (what DDP + torch.nn.utils.clip_grad_norm_ sees), the clipped update must equal one process on the whole batch, and the
(all-gathered, when sharded) EMA must equal the single-process one.  CPU only: the AdamW arithmetic is injected through the
host_update hook, the trainer computes the norm and the EMA with torch ops on CPU tensors."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

MAX_NORM = 0.05
DECAY = 0.9
EPS = 1e-3           # comparable to the clipped per-element gradients: AdamW is then far from scale-invariant
STEPS = 3


class TinyNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = nn.Conv2d(3, 8, 3, padding=1)
        self.enc = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1), nn.GELU(), nn.Conv2d(8, 8, 1))
        self.dec = nn.Sequential(nn.Conv2d(16, 8, 1), nn.GELU())
        self.out = nn.Conv2d(8, 3, 3, padding=1, bias=False)
        self.register_buffer("offset", torch.full((1, 3, 1, 1), 0.25))

    def forward(self, x):
        e = self.embed(x)
        h = self.enc(e)
        return self.out(self.dec(torch.cat([h, e], 1))) + x + self.offset


def _host_adamw(tr, scale):
    """AdamW on flat host buffers (stands in for the fused HIP kernel; the product has no CPU update)."""
    g = tr.flat_g * scale
    b1, b2 = tr.betas
    tr.flat_p.mul_(1.0 - tr.lr * tr.wd)
    tr.flat_m.mul_(b1).add_(g, alpha=1 - b1)
    tr.flat_v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** tr.step_count, math.sqrt(1 - b2 ** tr.step_count)
    tr.flat_p.addcdiv_(tr.flat_m, tr.flat_v.sqrt() / bc2 + tr.eps, value=-tr.lr / bc1)


def _data():
    g = torch.Generator().manual_seed(1)
    return torch.randn(4, 3, 8, 8, generator=g), torch.randn(4, 3, 8, 8, generator=g)


def _reference(clip=True):
    """One process, whole batch: torch clip_grad_norm_ + torch.optim.AdamW + BasicSR's model_ema."""
    torch.manual_seed(0)
    ref = TinyNet()
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-2, eps=EPS)
    ema = {k: v.detach().clone() for k, v in ref.named_parameters()}
    x, y = _data()
    norms = []
    for _ in range(STEPS):
        opt.zero_grad()
        (ref(x) - y).abs().mean().backward()
        if clip:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), MAX_NORM)))
        opt.step()
        with torch.no_grad():
            for k, p in ref.named_parameters():
                ema[k].mul_(DECAY).add_(p, alpha=1 - DECAY)
    return ref, ema, norms


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, mode, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from image_restoration_amd.trainer import FlatTrainer
        torch.manual_seed(0)
        model = TinyNet()
        sharded = mode == "sharded"
        tr = FlatTrainer(model, lr=1e-2, eps=EPS, overlap=mode == "overlap", host_update=_host_adamw, shard_optimizer=sharded,
                         max_grad_norm=MAX_NORM, ema_decay=DECAY)
        assert tr.sharded == sharded and tr.overlap == (mode == "overlap")
        assert tr.flat_ema.numel() == tr.shard
        x, y = _data()
        xs, ys = x[rank * 2:(rank + 1) * 2], y[rank * 2:(rank + 1) * 2]
        norms = []
        for _ in range(STEPS):
            tr.zero_grad()
            (model(xs) - ys).abs().mean().backward()
            tr.reduce_gradients()
            tr.optimizer_step()
            norms.append(float(tr.grad_norm))
        ema_sd = tr.ema_state_dict()                      # a collective when sharded: every rank calls it
        ret[f"norms{rank}"] = norms
        if rank == 0:
            ret["params"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
            ret["ema"] = ema_sd
            ret["keys"] = list(model.state_dict())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["overlap", "after_backward", "sharded"])
def test_two_rank_clipping_and_ema_match_single_process(mode):
    ref, ema_ref, norms_ref = _reference()
    unclipped, _, _ = _reference(clip=False)
    # the clip binds: without it the update is visibly different (the comparison below is not vacuous)
    assert max(float((a - b).abs().max()) for a, b in zip(ref.state_dict().values(), unclipped.state_dict().values())) > 1e-4
    assert min(norms_ref) > MAX_NORM
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), mode, ret), nprocs=2, join=True)
    assert ret["norms0"] == ret["norms1"], "the ranks disagree on the gradient norm"
    for got, want in zip(ret["norms0"], norms_ref):
        assert got == pytest.approx(want, rel=1e-5)
    for k, v in ref.state_dict().items():
        assert torch.allclose(ret["params"][k], v, rtol=1e-5, atol=1e-6), k
    ema = ret["ema"]
    assert list(ema) == ret["keys"]
    for k, v in ema_ref.items():
        assert torch.allclose(ema[k], v, rtol=1e-5, atol=1e-6), k
    assert torch.equal(ema["offset"], ref.offset)         # buffers come from the model
    # after 3 steps at decay 0.9 the average still sits visibly between the initial and the trained weights
    assert not torch.allclose(ema["out.weight"], ret["params"]["out.weight"], rtol=0, atol=1e-5)


def test_single_process_cpu_checkpoint_and_validation():
    """Constructor validation and the checkpoint rules, on the host path (no collectives)."""
    from image_restoration_amd.trainer import FlatTrainer
    torch.manual_seed(0)
    with pytest.raises(ValueError, match="2-norm"):
        FlatTrainer(TinyNet(), host_update=_host_adamw, max_grad_norm=1.0, norm_type=float("inf"))
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatTrainer(TinyNet(), host_update=_host_adamw, max_grad_norm=0.0)
    with pytest.raises(ValueError, match="ema_decay"):
        FlatTrainer(TinyNet(), host_update=_host_adamw, ema_decay=1.0)
    model = TinyNet()
    tr = FlatTrainer(model, lr=1e-2, host_update=_host_adamw, max_grad_norm=MAX_NORM, ema_decay=DECAY)
    assert torch.equal(tr.flat_ema, tr.flat_p)
    x, y = _data()
    for _ in range(2):
        tr.zero_grad()
        (model(x) - y).abs().mean().backward()
        tr.reduce_gradients()
        tr.optimizer_step()
    sd = tr.state_dict()
    assert sd["ema_decay"] == DECAY and sd["max_grad_norm"] == MAX_NORM and torch.equal(sd["ema"], tr.flat_ema)
    plain = FlatTrainer(TinyNet(), host_update=_host_adamw)
    assert not {"ema", "ema_decay", "max_grad_norm"} & set(plain.state_dict())
    with pytest.raises(ValueError, match="EMA"):
        plain.load_state_dict(sd)
    m2 = TinyNet()
    tr2 = FlatTrainer(m2, host_update=_host_adamw, ema_decay=0.5)
    m2.load_state_dict(model.state_dict())
    tr2.load_state_dict(sd)
    assert tr2.ema_decay == DECAY and torch.equal(tr2.flat_ema, tr.flat_ema) and tr2.step_count == 2
    tr2.load_state_dict(plain.state_dict() | {"numel": tr2.total})  # an older state without EMA: restart it at the weights
    assert torch.equal(tr2.flat_ema, tr2.flat_p)
    with tr.ema_weights():
        assert torch.equal(tr.flat_p, tr.flat_ema)
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.optimizer_step()
    assert torch.equal(tr.flat_p, tr2.flat_p)

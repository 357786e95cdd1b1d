"""Cost of gradient-norm clipping and the weight EMA (FlatTrainer(max_grad_norm=..., ema_decay=...)).

Part 1, kernels at Restormer base's flat parameter size (26.1 M fp32), device events around OPT_ITERS launches, median of OPT_REPS:
  adamw        mi_adamw_step                                   (28n bytes)
  sumsq        mi_grad_sumsq alone                             (4n)
  clip         mi_grad_sumsq + mi_adamw_step_ex with clipping  (4n + 28n)
  ema          mi_adamw_step_ex with the EMA                   (36n)
  clip_ema     mi_grad_sumsq + mi_adamw_step_ex with both      (4n + 36n)
Part 2, a Restormer base training step (bs OPT_BATCH x 256^2, bf16, eager, as bench.py) with max_grad_norm=0.01,
ema_decay=0.999 against the same trainer with both switched off, alternating blocks of OPT_STEPS steps in one process.
Prints one JSON line.  Run on the GPU box: python tools/bench_optim.py   (OPT_SKIP_STEP=1: kernels only)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_restoration_amd as m  # noqa: E402
from image_restoration_amd import configs, ops  # noqa: E402
from image_restoration_amd.trainer import ALIGN, FlatTrainer  # noqa: E402

DEV = "cuda"
ITERS = int(os.environ.get("OPT_ITERS", "50"))
REPS = int(os.environ.get("OPT_REPS", "7"))
BATCH = int(os.environ.get("OPT_BATCH", "32"))
STEPS = int(os.environ.get("OPT_STEPS", "10"))
ROUNDS = int(os.environ.get("OPT_ROUNDS", "3"))


def time_us(fn):
    """Median over REPS of the mean device time of ITERS back-to-back calls (us)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / ITERS * 1e3)
    return statistics.median(out)


def kernels():
    net = m.Restormer(**configs.RESTORMER_BASE)
    n = sum((p.numel() + ALIGN - 1) // ALIGN * ALIGN for p in net.parameters())
    del net
    g = torch.Generator().manual_seed(0)
    p = (0.02 * torch.randn(n, generator=g)).to(DEV)
    grad = (1e-4 * torch.randn(n, generator=g)).to(DEV)
    mom, var, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    ss, norm = torch.zeros(1, device=DEV), torch.zeros((), device=DEV)
    ws = ops.grad_sumsq_workspace(n, DEV)
    dsc = torch.tensor([2e-4, 0.1, 0.03], device=DEV)       # lr, bias corrections from the device, as a captured step
    hp = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, dev_scalars=dsc)

    def adamw():
        ops.adamw_step(p, grad, mom, var, 2e-4, 1, **hp)

    def sumsq():
        ops.grad_sumsq(grad, ss, ws)

    def clip():
        ops.grad_sumsq(grad, ss, ws)
        ops.adamw_step_ex(p, grad, mom, var, 2e-4, 1, **hp, sumsq=ss, max_norm=0.01, norm_out=norm)

    def ema_only():
        ops.adamw_step_ex(p, grad, mom, var, 2e-4, 1, **hp, ema=ema, ema_decay=0.999)

    def clip_ema():
        ops.grad_sumsq(grad, ss, ws)
        ops.adamw_step_ex(p, grad, mom, var, 2e-4, 1, **hp, sumsq=ss, max_norm=0.01, norm_out=norm, ema=ema, ema_decay=0.999)

    res = {"n": n}
    for name, fn, nbytes in (("adamw", adamw, 28), ("sumsq", sumsq, 4), ("clip", clip, 32), ("ema", ema_only, 36),
                             ("clip_ema", clip_ema, 40)):
        us = time_us(fn)
        res[name] = {"us": round(us, 1), "TB/s": round(nbytes * n / (us * 1e-6) / 1e12, 2)}
    res["extra_us_clip_ema"] = round(res["clip_ema"]["us"] - res["adamw"]["us"], 1)
    return res


def step_ab():
    torch.manual_seed(0)
    net = m.Restormer(**configs.RESTORMER_BASE).to(DEV)
    tr = FlatTrainer(net, lr=2e-4, max_grad_norm=0.01, ema_decay=0.999)
    gen = torch.Generator().manual_seed(1234)
    clean = torch.rand((BATCH, 3, 256, 256), generator=gen)
    noisy = torch.clamp(clean + 0.1 * torch.randn(clean.shape, generator=gen), 0, 1)
    clean, noisy = clean.to(DEV).to(torch.bfloat16), noisy.to(DEV).to(torch.bfloat16)
    on_state = (tr.max_grad_norm, tr.flat_ema)

    def set_on(on):
        # one trainer, so that both legs share the model, the activations and the library's caches; "off" is exactly the
        # default step (optimizer_step launches mi_adamw_step when both features are None)
        tr.max_grad_norm, tr.flat_ema = on_state if on else (None, None)

    def step():
        tr.zero_grad()
        out = net(noisy)
        _, dout = ops.l1_loss(out, clean, want_grad=True)
        out.backward(dout)
        tr.reduce_gradients()
        tr.optimizer_step()

    for on in (True, False):
        set_on(on)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {True: [], False: []}
    for _ in range(ROUNDS):
        for on in (False, True):
            set_on(on)
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                step()
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / STEPS * 1e3)
    set_on(True)
    tr.close()
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {"batch": BATCH, "off_ms": round(off, 2), "on_ms": round(on, 2), "delta_ms": round(on - off, 3),
            "off_all": [round(x, 2) for x in ms[False]], "on_all": [round(x, 2) for x in ms[True]]}


def main():
    assert torch.cuda.is_available(), "tools/bench_optim.py needs the MI355X"
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernels()}
    if os.environ.get("OPT_SKIP_STEP") != "1":
        res["step"] = step_ab()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Times forward plus gradient of the native SSIM, edge and focal-L1 loss terms (losses.SSIMloss / EdgeLoss / FocalL1Loss:
mi_ssim_loss, mi_edge_loss, mi_focal_l1_loss) against the same formulas composed from torch ops with autograd - what a user
would write without them: F.conv2d for the two windows (MIOpen), elementwise ops for the rest, inputs widened to fp32 - at the
two training shapes, 32x3x256x256 and 8x3x128x128, in bf16 and fp32.  Both paths run in the same process, alternating, after
a warm-up of each; every sample is a device-event window over PL_ITERS calls (loss.backward() included), and the figure kept is
the median of PL_SAMPLES windows with the fastest and slowest beside it.  The two results are compared before anything is
timed.  Run on the GPU:  python tools/bench_losses.py   (a table on stderr for DESIGN.md, one JSON line on stdout)."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_restoration_amd import losses  # noqa: E402

DEV = "cuda"
SHAPES = [(32, 3, 256, 256), (8, 3, 128, 128)]
ITERS = int(os.environ.get("PL_ITERS", "50"))
SAMPLES = int(os.environ.get("PL_SAMPLES", "7"))
WARM = int(os.environ.get("PL_WARM", "5"))


def torch_ssim_loss(pred, target):
    x, y = pred.float(), target.float()
    c = x.shape[1]
    g = torch.exp(-(torch.arange(11, dtype=torch.float32, device=x.device) - 5) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    gv, gh = g.view(1, 1, 11, 1).expand(c, 1, 11, 1), g.view(1, 1, 1, 11).expand(c, 1, 1, 11)
    win = lambda t: F.conv2d(F.conv2d(t, gv, groups=c), gh, groups=c)
    mu1, mu2 = win(x), win(y)
    s1, s2, s12 = win(x * x) - mu1 * mu1, win(y * y) - mu2 * mu2, win(x * y) - mu1 * mu2
    S = (2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
    return 1 - S.mean()


def torch_edge_loss(pred, target):
    d = pred.float() - target.float()
    c = d.shape[1]
    k = torch.tensor([[.05, .25, .4, .25, .05]], device=d.device)
    k2 = torch.matmul(k.t(), k).expand(c, 1, 5, 5)
    blur = lambda t: F.conv2d(F.pad(t, (2, 2, 2, 2), mode="replicate"), k2, groups=c)
    z = torch.zeros_like(d)
    z[:, :, ::2, ::2] = 4 * blur(d)[:, :, ::2, ::2]
    e = d - blur(z)
    return (e * e).mean()


def torch_focal_loss(pred, target):
    a = (pred.float() - target.float()).abs() / 0.1
    return (torch.log1p(a + 1e-6) ** 2.0 * a).mean()


TERMS = {"ssim": (losses.SSIMloss(), torch_ssim_loss), "edge": (losses.EdgeLoss(), torch_edge_loss),
         "focal_l1": (losses.FocalL1Loss(), torch_focal_loss)}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_losses: no GPU (there is nothing to measure on a CPU)")
    log = lambda *a: print(*a, file=sys.stderr, flush=True)
    log(f"# {torch.cuda.get_device_name(0)}; {SAMPLES} windows of {ITERS} calls per figure, {WARM} warm-up calls; us per call, "
        "forward + gradient")
    log("| term | shape | dtype | native: median (min .. max) | torch ops + autograd: median (min .. max) | native / torch | "
        "loss difference | gradient difference |")
    log("|---|---|---|---|---|---|---|---|")
    rows = []
    for shape in SHAPES:
        for dtype in (torch.bfloat16, torch.float32):
            g = torch.Generator(device="cpu").manual_seed(5)
            target = torch.rand(shape, generator=g).to(DEV).to(dtype)
            pred = (target.float() + 0.05 * torch.randn(shape, generator=g).to(DEV)).clamp(0, 1).to(dtype).requires_grad_(True)
            for term, (native, composed) in TERMS.items():
                fns = {}
                for name, f in (("native", native), ("torch", composed)):
                    def step(f=f):
                        pred.grad = None
                        loss = f(pred, target)
                        loss.backward()
                        return loss
                    fns[name] = step
                res = {}
                for name, fn in fns.items():
                    for _ in range(WARM):
                        loss = fn()
                    res[name] = (float(loss.detach()), pred.grad.double().clone())
                torch.cuda.synchronize()
                dl = abs(res["native"][0] - res["torch"][0]) / abs(res["torch"][0])
                dg = float((res["native"][1] - res["torch"][1]).norm() / res["torch"][1].norm())
                t = {name: [] for name in fns}
                for _ in range(SAMPLES):                    # alternate the two paths: drift hits both alike
                    for name, fn in fns.items():
                        t[name].append(window(fn, ITERS))
                med = {k: statistics.median(v) for k, v in t.items()}
                fmt = lambda k: f"{med[k]:.0f} ({min(t[k]):.0f} .. {max(t[k]):.0f})"
                sh, dn = "x".join(map(str, shape)), str(dtype).split(".")[-1]
                log(f"| {term} | {sh} | {dn} | {fmt('native')} | {fmt('torch')} | {med['native'] / med['torch']:.2f} | {dl:.1e} | {dg:.1e} |")
                rows.append({"term": term, "shape": sh, "dtype": dn, "native_us": round(med["native"], 1),
                             "native_min_us": round(min(t["native"]), 1), "native_max_us": round(max(t["native"]), 1),
                             "torch_us": round(med["torch"], 1), "torch_min_us": round(min(t["torch"]), 1),
                             "torch_max_us": round(max(t["torch"]), 1), "loss_rel_diff": dl, "grad_rel_diff": dg})
    print(json.dumps({"bench": "pixel_losses", "device": torch.cuda.get_device_name(0), "iters": ITERS, "samples": SAMPLES,
                      "unit": "us per forward + gradient call", "rows": rows}))


if __name__ == "__main__":
    main()

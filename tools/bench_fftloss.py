"""Times the FFT loss, forward plus gradient, on the native path (FFTLoss(native=True): mi_fft_l1_loss, dense-DFT GEMMs on the fp32
MFMA) and on the default path (torch.fft.rfft2 into rocFFT, mi_l1_loss, autograd's backward) at the two training shapes,
32x3x256x256 and 8x3x128x128, in fp32 and bf16.  Both paths run in the same process, alternating, after a warm-up of each; every
sample is a device-event window over FL_ITERS calls (loss.backward() included), and the figure printed is the median of
FL_SAMPLES windows with the fastest and slowest beside it.  The two results are compared before anything is timed.
Run on the GPU:  python tools/bench_fftloss.py   (prints a markdown table for DESIGN.md 7i)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_restoration_amd import ops  # noqa: E402
from image_restoration_amd.losses import FFTLoss  # noqa: E402

DEV = "cuda"
SHAPES = [(32, 3, 256, 256), (8, 3, 128, 128)]
ITERS = int(os.environ.get("FL_ITERS", "20"))
SAMPLES = int(os.environ.get("FL_SAMPLES", "9"))
WARM = int(os.environ.get("FL_WARM", "5"))


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
        raise SystemExit("bench_fftloss: no GPU (there is nothing to measure on a CPU)")
    print(f"# {torch.cuda.get_device_name(0)}; {SAMPLES} windows of {ITERS} calls per figure, {WARM} warm-up calls; us per call")
    print("| shape | dtype | native fwd+grad: median (min .. max) | rocFFT + autograd fwd+grad: median (min .. max) | "
          "native / rocFFT | native launches | loss difference |")
    print("|---|---|---|---|---|---|---|")
    for shape in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device="cpu").manual_seed(5)
            pred = torch.rand(shape, generator=g).to(DEV).to(dtype).requires_grad_(True)
            target = torch.rand(shape, generator=g).to(DEV).to(dtype)
            fns = {}
            for name, mod in (("native", FFTLoss(native=True)), ("rocfft", FFTLoss())):
                def step(mod=mod):
                    pred.grad = None
                    loss = mod(pred, target)
                    loss.backward()
                    return loss
                fns[name] = step
            losses = {}
            for name, fn in fns.items():
                for _ in range(WARM):
                    losses[name] = fn()
            torch.cuda.synchronize()
            diff = abs(losses["native"].item() - losses["rocfft"].item()) / abs(losses["rocfft"].item())
            t = {name: [] for name in fns}
            for _ in range(SAMPLES):                    # alternate the two paths: drift hits both alike
                for name, fn in fns.items():
                    t[name].append(window(fn, ITERS))
            med = {k: statistics.median(v) for k, v in t.items()}
            fmt = lambda k: f"{med[k]:.0f} ({min(t[k]):.0f} .. {max(t[k]):.0f})"
            plan = ops.fft_l1_plan(*shape, dtype, True)
            print(f"| {'x'.join(map(str, shape))} | {str(dtype).split('.')[-1]} | {fmt('native')} | {fmt('rocfft')} | "
                  f"{med['native'] / med['rocfft']:.2f} | {plan['launches']} | {diff:.1e} |", flush=True)


if __name__ == "__main__":
    main()

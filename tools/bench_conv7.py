"""7x7 reflect conv (rpst_conv7) timings per LDMSAdaINRPNet encoder layer (one MI355X).

    python tools/bench_conv7.py [--n 8] [--size 512] [--rounds 3] [--out profiles/ld_adain/conv7.json]

Per layer C -> C (32, 64, 128, 256) at (N, C, size, size), in the same process, alternating,
after a warm-up: `rounds` timed windows (HIP events on the launch stream) of enough calls to
fill about 0.3 s each, the median window per call reported with the windows' min / max:
  conv7      ops.conv2d_k7, reflect pad 3, LeakyReLU, bias    FLOP = 2 C C 49 H W N
  direct3x3  ops.conv2d, reflect pad 1, the direct MFMA kernel (RPST_CONV_ALGO=direct) at
             the same channels / size / N                     FLOP = 2 C C 9 H W N
  torch7x7   F.leaky_relu(F.conv2d(F.pad(x, (3,)*4, 'reflect'), w, b)) on the GPU (MIOpen)
TF/s are those FLOP over the median, `frac` their share of the 157.3 TF/s fp32 MFMA peak
(both convs are compute-bound at these shapes: the bytes are < 1 % of the time at peak)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rp-style-transfer_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_TFLOPS = 157.3
CHANNELS = (32, 64, 128, 256)


def window(fn, reps):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def medians(fns, rounds, target_ms=300.0):
    """name -> (median, min, max, reps) ms per call over `rounds` windows, alternating."""
    reps = {}
    for k, fn in fns.items():  # warm-up: code objects, allocator, MIOpen's choice
        fn()
        reps[k] = max(2, min(200, int(target_ms / max(window(fn, 1), 1e-3))))
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, reps[k]))
    return {k: (statistics.median(v), min(v), max(v), reps[k]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv7: needs a ROCm GPU")
    from rpst import ops
    dev = torch.device("cuda:0")
    n, hw = args.n, args.size
    rows = []
    for c in args.channels:
        g = torch.Generator(device=dev).manual_seed(c)
        x = torch.rand((n, c, hw, hw), device=dev, generator=g) - 0.5
        w7 = (torch.rand((c, c, 7, 7), device=dev, generator=g) - 0.5) * (12.0 / (c * 49)) ** 0.5
        w3 = (torch.rand((c, c, 3, 3), device=dev, generator=g) - 0.5) * (12.0 / (c * 9)) ** 0.5
        b = torch.rand((c,), device=dev, generator=g) - 0.5
        p7, p3 = ops.pack_conv7_weight(w7), ops.pack_conv_weight(w3)
        out = torch.empty_like(x)

        def conv7():
            ops.conv2d_k7(x, p7, b, c, pad=ops.PAD_REFLECT, act=ops.ACT_LRELU, out=out)

        def direct3():
            os.environ["RPST_CONV_ALGO"] = "direct"
            try:
                ops.conv2d(x, p3, b, c, 3, pad=ops.PAD_REFLECT, relu=ops.ACT_LRELU, out=out)
            finally:
                del os.environ["RPST_CONV_ALGO"]

        def torch7():
            F.leaky_relu(F.conv2d(F.pad(x, (3,) * 4, mode="reflect"), w7, b), 0.2)

        fns = {"conv7": conv7, "direct3x3": direct3}
        if not args.no_torch:
            fns["torch7x7"] = torch7
        with torch.no_grad():
            os.environ["RPST_CONV_ALGO"] = "direct"
            algo = ops.conv_algorithm(c, c, hw, hw, 3, ops.IN_NONE)
            del os.environ["RPST_CONV_ALGO"]
            assert algo == ops.ALGO_DIRECT, algo
            res = medians(fns, args.rounds)
            # the two 7x7 paths agree (same inputs, fp32)
            ops.conv2d_k7(x[:1], p7, b, c, pad=ops.PAD_REFLECT, act=ops.ACT_LRELU, out=out[:1])
            ref = F.leaky_relu(F.conv2d(F.pad(x[:1], (3,) * 4, mode="reflect"), w7, b), 0.2)
            agree = float((out[:1] - ref).norm() / ref.norm())
        for k, (med, lo, hi, reps) in res.items():
            taps = 9 if k == "direct3x3" else 49
            flop = 2.0 * c * c * taps * hw * hw * n
            tf = flop / med / 1e9
            r = {"op": k, "shape": [n, c, hw, hw], "ms": round(med, 4), "ms_min": round(lo, 4),
                 "ms_max": round(hi, 4), "reps": reps, "rounds": args.rounds,
                 "TFps": round(tf, 2), "frac_of_157.3": round(tf / PEAK_TFLOPS, 4)}
            if k == "conv7":
                r["rel_l2_vs_torch"] = agree
            print(json.dumps(r), flush=True)
            rows.append(r)
        del x, out, w7, w3, p7, p3
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

"""Masked AdaIN timings next to the unmasked op (one MI355X).

    python tools/bench_masked.py [--reps 20] [--rounds 5] [--out profiles/masked_adain/bench.json]

ops.masked_adain and ops.adaptive_instance_normalization at the same shapes in the same
process, alternating, after a warm-up of every shape: `rounds` timed windows of `reps` calls
each (HIP events on the launch stream), the median window per call reported. The unmasked op
moves the same bytes but for 1 B/pixel of labels, so it is the yardstick. GB/s are algorithmic
bytes over the median: AdaIN 3 planes of fp32 (content, style read; out written); masked AdaIN
the same plus the content labels read twice and the style labels once. The masked op is also
timed in its parts (plan, params, apply) and with a skip tensor (one more plane read).

Then MultiScaleAdaINRPNet.test at 512x512 with bench.py's MULTISCALE_CONFIG, use_mask True
(label maps already on the device) against False. Writes all rows as one JSON document."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rp-style-transfer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(1, 32, 512, 512), (8, 32, 512, 512), (8, 512, 64, 64)]
LABELS = [1, 4, 16]


def label_map(n, h, w, labels, seed):
    """Piecewise-constant maps: a grid of rectangles with `labels` labels, each image its
    own arrangement."""
    rng = np.random.default_rng(seed)
    g = int(np.ceil(np.sqrt(labels)))
    out = np.zeros((n, h, w), dtype=np.uint8)
    ys, xs = np.linspace(0, h, g + 1).astype(int), np.linspace(0, w, g + 1).astype(int)
    for b in range(n):
        order = rng.permutation(g * g) % labels
        for j in range(g):
            for i in range(g):
                out[b, ys[j]:ys[j + 1], xs[i]:xs[i + 1]] = order[j * g + i]
    return torch.from_numpy(out)


def window(fn, reps):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def medians(fns, reps, rounds):
    """name -> median ms per call over `rounds` windows, the candidates alternating."""
    for fn in fns.values():  # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, reps))
    return {k: statistics.median(v) for k, v in times.items()}, \
        {k: (min(v), max(v)) for k, v in times.items()}


def bench_ops(dev, reps, rounds):
    from rpst import ops
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for shape in SHAPES:
        n, c, h, w = shape
        x = torch.rand(shape, device=dev, generator=g)
        y = torch.rand(shape, device=dev, generator=g) * 2 + 1
        skip = torch.rand(shape, device=dev, generator=g)
        out = torch.empty_like(x)
        plane_bytes = 4.0 * n * c * h * w
        for labels in LABELS:
            cseg = label_map(n, h, w, labels, 1).to(dev)
            sseg = label_map(n, h, w, labels, 2).to(dev)
            plan = ops.segment_plan(cseg, sseg)
            fns = {
                "adain": lambda: ops.adaptive_instance_normalization(x, y, out=out),
                "masked_adain": lambda: ops.masked_adain(x, y, cseg, sseg, out=out),
                "masked_adain_skip": lambda: ops.masked_adain(x, y, cseg, sseg, skip=skip,
                                                              plan=plan, out=out),
                "segment_plan": lambda: ops.segment_plan(cseg, sseg),
                "masked_params": lambda: ops.masked_adain_params(x, y, cseg, sseg, plan=plan),
            }
            med, spread = medians(fns, reps, rounds)
            seg_bytes = float(n * h * w)
            nbytes = {"adain": 3 * plane_bytes,
                      "masked_adain": 3 * plane_bytes + 2 * seg_bytes * c + seg_bytes * c,
                      "masked_adain_skip": 4 * plane_bytes + 3 * seg_bytes * c,
                      "segment_plan": 2 * seg_bytes,
                      "masked_params": 2 * plane_bytes + 2 * seg_bytes * c}
            for k in fns:
                rows.append({"op": k, "shape": list(shape), "labels": labels,
                             "ms": round(med[k], 4), "ms_min": round(spread[k][0], 4),
                             "ms_max": round(spread[k][1], 4),
                             "GBps": round(nbytes[k] / med[k] / 1e6, 1)})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_net(dev, reps, rounds):
    import bench
    import network as net
    from rpst import synth
    rows = []
    c = torch.from_numpy(synth.image(1, (1, 3, 512, 512))).to(dev)
    s = torch.from_numpy(synth.image(2, (1, 3, 512, 512))).to(dev)
    cseg, sseg = label_map(1, 512, 512, 4, 1).to(dev), label_map(1, 512, 512, 4, 2).to(dev)
    models = {}
    for masked in (False, True):
        m = net.MultiScaleAdaINRPNet(dict(bench.MULTISCALE_CONFIG, use_mask=masked),
                                     copy.deepcopy(net.vgg))
        synth.synth_module_(m, 10)
        models[masked] = m.to(dev)
    fns = {"multiscale_test": lambda: models[False].test(c, s),
           "multiscale_test_masked": lambda: models[True].test(c, s, c_mask_path=cseg,
                                                               s_mask_path=sseg)}
    med, spread = medians(fns, reps, rounds)
    for k in fns:
        rows.append({"op": k, "shape": [1, 3, 512, 512], "labels": 4, "ms": round(med[k], 4),
                     "ms_min": round(spread[k][0], 4), "ms_max": round(spread[k][1], 4)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_adain", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_masked: no GPU (timings are taken on the MI355X only)")
    dev = torch.device("cuda:0")
    rows = bench_ops(dev, a.reps, a.rounds) + bench_net(dev, a.reps, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""LDMSAdaINRPNet.test() (`network: ld_adain`) throughput at the reference's config (one MI355X).

    python tools/bench_ld.py [--n 4] [--size 512] [--rounds 3] [--reps 2] [--out profiles/ld_adain/ld.json]

hidden_dim 16, ld_layer_num 5, unmasked, synthetic weights, N content / style pairs (the
level-4 feature is 512 channels: 537 MB per image at 512^2, over 2N images). After a warm-up,
`rounds` windows of `reps` test() calls (HIP events on the launch stream); images/s from the
median window. Then one traced test() (rpst.ops.TRACE: HIP events around every library call)
gives the time in the four 7x7 launches and their share of the traced step."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rp-style-transfer_amd"))

import torch  # noqa: E402

CONFIG = {"rp_blocks": 5, "hidden_dim": 16, "content_weight": 1.0, "style_weight": 10.0,
          "resume": False, "use_mask": False, "shuffle": False, "shuffle_layers": 1,
          "sort": False, "stylized_layers": 5, "enc_stack_way": "NONE", "inception_num": 0,
          "attention": "none", "ld_layer_num": 5}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ld: needs a ROCm GPU")
    import network as net
    from rpst import ops, synth
    dev = torch.device("cuda:0")
    m = net.LDMSAdaINRPNet(CONFIG, copy.deepcopy(net.vgg))
    synth.synth_module_(m, 3)
    m = m.to(dev)
    shape = (args.n, 3, args.size, args.size)
    c = torch.from_numpy(synth.image(1, shape)).to(dev)
    s = torch.from_numpy(synth.image(2, shape)).to(dev)
    for _ in range(2):  # warm-up: code objects, packed weights, allocator
        y = m.test(c, s)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    times = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            m.test(c, s)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / args.reps)
    med = statistics.median(times)
    ops.TRACE = ops.Trace()
    try:
        m.test(c, s)
        summary = ops.TRACE.summary()
    finally:
        ops.TRACE = None
    traced = sum(v["ms"] for v in summary.values())
    k7 = {k: v for k, v in summary.items() if k.startswith("conv7x7 ")}
    k7_ms = sum(v["ms"] for v in k7.values())
    k7_flop = sum(v["flops"] * v["launches"] for v in k7.values())
    row = {"op": "LDMSAdaINRPNet.test", "hidden": 16, "layers": 5, "shape": list(shape),
           "ms": round(med, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
           "rounds": args.rounds, "reps": args.reps, "img_per_s": round(args.n / med * 1e3, 3),
           "traced_step_ms": round(traced, 3), "conv7_ms": round(k7_ms, 3),
           "conv7_launches": sum(v["launches"] for v in k7.values()),
           "conv7_share_of_traced_step": round(k7_ms / traced, 4),
           "conv7_TFps": round(k7_flop / k7_ms / 1e9, 2)}
    print(json.dumps(row), flush=True)
    layers = [{"op": k, "ms": round(v["ms"], 3), "launches": v["launches"],
               "share_of_traced_step": round(v["ms"] / traced, 4)}
              for k, v in sorted(summary.items(), key=lambda kv: -kv[1]["ms"])]
    for r in layers[:12]:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"result": row, "launches": layers}, f, indent=1)


if __name__ == "__main__":
    main()

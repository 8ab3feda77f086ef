"""LDMSAdaINRPNet4.test() (`network: ld_adain4`) throughput at the reference's config (one
MI355X), and the three kernels between its encoders and its decoder against HBM.

    python tools/bench_ld4.py [--n 4] [--size 512] [--rounds 5] [--reps 3] [--context]
                              [--out profiles/ld4/bench.json]

hidden_dim 32, ld_layer_num 5, stylized_layers 1 (train_ld4_multiscale_rp_adain.yaml), synthetic
weights, N content / style pairs. Three routes of test(), their windows alternating after a
warm-up (`rounds` windows of `reps` calls each, HIP events on the launch stream; images/s from
the median window): the fused route (no masks), the same step with the AdaIN fusion off
(op by op: levels, AdaIN outputs and concatenations written), and `use_mask: True` with four
labels per image. One traced step per route (rpst.ops.TRACE: HIP events around every library
call) gives the time and the launches of rpst_ld4_fuse / rpst_resized_mean_std /
rpst_resize_nearest inside it; their GB/s come from stand-alone windows of each launch shape of
the step (a single traced launch includes the host gap before it). Bytes are algorithmic: what
the op must read plus what it must write (ops.py's trace entries).

--context also records, from child processes run before anything else here, tools/bench_adain.py's
GB/s for rpst_adain at 64 channels and tools/bench_ld.py's images/s at the same N and size."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rp-style-transfer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

CONFIG = {"rp_blocks": 5, "hidden_dim": 32, "content_weight": 1.0, "style_weight": 1.0,
          "resume": False, "use_mask": False, "shuffle": False, "shuffle_layers": 1,
          "sort": False, "stylized_layers": 1, "enc_stack_way": "NONE", "inception_num": 0,
          "attention": "none", "ld_layer_num": 5}
NEW_KERNELS = ("ld4_fuse", "resized_mean_std", "resize_nearest")


def child_rows(script, *args):
    """The JSON lines a sibling benchmark prints, run as a child process."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", script), *args],
                         check=True, capture_output=True, text=True).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def traced(fn):
    from rpst import ops
    ops.TRACE = ops.Trace()
    try:
        fn()
        return ops.TRACE.summary()
    finally:
        ops.TRACE = None


def kernel_rows(summary):
    """Per new kernel: launches and time inside one traced step."""
    total = sum(v["ms"] for v in summary.values())
    rows = {"traced_step_ms": round(total, 3)}
    for kern in NEW_KERNELS:
        hit = {k: v for k, v in summary.items() if k.startswith(kern + " ")}
        if hit:
            ms = sum(v["ms"] for v in hit.values())
            rows[kern] = {"launches": sum(v["launches"] for v in hit.values()),
                          "ms": round(ms, 3), "share_of_traced_step": round(ms / total, 4),
                          "MB": round(sum(v["bytes"] * v["launches"] for v in hit.values()) / 1e6, 1)}
    return rows


def standalone(n, size, reps, rounds):
    """Each launch shape of the fused step (and the op-by-op level's resize) on its own:
    median window -> ms and GB/s of algorithmic bytes."""
    from bench_masked import window
    from rpst import ops
    dev = torch.device("cuda:0")
    h = CONFIG["hidden_dim"]
    g = torch.Generator(device=dev).manual_seed(0)
    fine = torch.rand((2 * n, h, size, size), device=dev, generator=g)
    y = torch.rand((n, h, size, size), device=dev, generator=g)
    par = torch.rand(4 * n * h, device=dev, generator=g) + 0.5
    level = torch.empty((2 * n, 2 * h, size, size), device=dev)
    rows = []
    for lv in range(CONFIG["ld_layer_num"]):
        cs = -(-size // 2 ** (lv + 1))
        coarse = torch.rand((2 * n, h, cs, cs), device=dev, generator=g)
        ca = 0 if lv == CONFIG["ld_layer_num"] - 1 else h
        out = torch.empty((n, ca + 2 * h, size, size), device=dev)
        fns = {
            "ld4_fuse": (lambda: ops.ld4_fuse(y if ca else None, fine, coarse, par, par, n=n,
                                              out=out),
                         4.0 * n * ((2 * ca + 3 * h) * size * size + h * cs * cs)),
            "resized_mean_std": (lambda: ops.resized_mean_std(coarse, (size, size)),
                                 4.0 * 2 * n * h * cs * cs),
            "resize_nearest": (lambda: ops.resize_nearest(coarse, (size, size), out=level,
                                                          out_channel_offset=h),
                               4.0 * 2 * n * h * (cs * cs + size * size)),
        }
        for fn, _ in fns.values():  # warm-up
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, (fn, _) in fns.items():
                times[k].append(window(fn, reps))
        for k, (_, nbytes) in fns.items():
            ms = statistics.median(times[k])
            rows.append({"op": k, "level": lv, "coarse": [cs, cs], "Ca": ca if k == "ld4_fuse" else None,
                         "ms": round(ms, 4), "ms_min": round(min(times[k]), 4),
                         "ms_max": round(max(times[k]), 4), "MB": round(nbytes / 1e6, 1),
                         "GBps": round(nbytes / ms / 1e6, 1)})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--context", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ld4: needs a ROCm GPU")
    doc = {}
    if args.context:  # children first: nothing of this process is on the GPU yet
        adain = child_rows("bench_adain.py", "--n", str(args.n), "--c", "64", "--hw",
                           str(args.size * args.size))
        ld = child_rows("bench_ld.py", "--n", str(args.n), "--size", str(args.size))
        doc["context"] = {"bench_adain": [r for r in adain if r["op"] == "adain"][0],
                          "bench_ld": ld[0]}
        print(json.dumps(doc["context"]), flush=True)
    import network as net
    import network.adain_rp as arp
    from bench_masked import label_map, window
    from rpst import synth
    dev = torch.device("cuda:0")
    models = {}
    for masked in (False, True):
        m = net.LDMSAdaINRPNet4(dict(CONFIG, use_mask=masked), copy.deepcopy(net.vgg))
        synth.synth_module_(m, 3)
        models[masked] = m.to(dev)
    shape = (args.n, 3, args.size, args.size)
    c = torch.from_numpy(synth.image(1, shape)).to(dev)
    s = torch.from_numpy(synth.image(2, shape)).to(dev)
    cseg = label_map(args.n, args.size, args.size, 4, 1).to(dev)
    sseg = label_map(args.n, args.size, args.size, 4, 2).to(dev)

    def unfused():
        arp.FUSED_ADAIN = False
        try:
            return models[False].test(c, s)
        finally:
            arp.FUSED_ADAIN = True

    routes = {"fused": lambda: models[False].test(c, s),
              "op_by_op": unfused,
              "masked": lambda: models[True].test(c, s, c_mask_path=cseg, s_mask_path=sseg)}
    outs = {}
    for k, fn in routes.items():  # warm-up: code objects, packed weights, allocator
        fn()
        outs[k] = fn()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in outs.values())
    diff = float((outs["fused"] - outs["op_by_op"]).norm() / outs["op_by_op"].norm())
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(window(fn, args.reps))
    doc["config"] = {"hidden": 32, "layers": 5, "stylized_layers": 1, "shape": list(shape),
                     "rounds": args.rounds, "reps": args.reps, "labels": 4}
    doc["routes"] = {}
    for k, fn in routes.items():
        med = statistics.median(times[k])
        row = {"ms": round(med, 3), "ms_min": round(min(times[k]), 3),
               "ms_max": round(max(times[k]), 3), "img_per_s": round(args.n / med * 1e3, 2)}
        row.update(kernel_rows(traced(fn)))
        doc["routes"][k] = row
        print(json.dumps({"route": k, **row}), flush=True)
    doc["fused_vs_op_by_op_rel_l2"] = diff
    del models, outs
    torch.cuda.empty_cache()
    doc["kernels"] = standalone(args.n, args.size, max(args.reps, 5), args.rounds)
    for r in doc["kernels"]:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

"""Opt-in bf16 inference against fp32: per-layer conv kernels and whole AdaINRPNet.test()
(rp_blocks 5, hidden 16) at BASELINE configs[1] (N = 32 content + 32 style, 512^2), one MI355X.

    python tools/bench_bf16.py [--n 32] [--size 512] [--rounds 3] [--out profiles/bf16/bench_bf16.json]

Everything runs in one process, interleaved: per layer and for the whole test() the order is
fp32 (a), bf16, fp32 (b), `rounds` times over, each a HIP-event window of enough calls to fill
about 0.3 s after a warm-up. Reported per entry: the median window per call in ms with the
windows' min / max. The fp32 measurement is taken twice (a, b) so that the run-to-run spread
is on record next to every fp32 / bf16 difference.

Layers are launched as the plans launch them: the encoder's 16->32 .. 64->128 over the
2N-image batch, its last conv 128->256 with the statistics epilogue storing the content half
(store_n = N), the decoder's first conv 256->128 through the AdaIN loader, the rest plain, all
zero padding + ReLU. fp32 = the kernel rpst_conv2d picks (ops.conv2d / conv2d_stats), bf16 =
ops.conv2d_bf16 whether or not ops.conv2d_bf16_supports keeps the layer (the column `kept`).
Per layer: direct-convolution FLOP = 2 N Cout Cin 9 H W over the bf16 time as a share of the
2.5 PF bf16 MFMA peak, and the fp32 activation bytes (input + stored output) over it as a
share of the 8 TB/s HBM peak.
"""
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

PEAK_BF16_TFLOPS = 2500.0
PEAK_HBM_GBPS = 8000.0


def window(fn, reps):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def interleaved(fns, rounds, target_ms=300.0):
    """name -> {"ms": median, "min", "max", "reps"} per call over `rounds` windows, the
    entries of fns alternating in their order."""
    reps = {}
    for k, fn in fns.items():  # warm-up: code objects, allocator, packed-weight caches
        fn()
        torch.cuda.synchronize()
        reps[k] = max(2, min(200, int(target_ms / max(window(fn, 1), 1e-3))))
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, reps[k]))
    return {k: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4),
                "max": round(max(v), 4), "reps": reps[k]} for k, v in times.items()}


def layer_row(ops, dev, n, cin, cout, size, form, rounds):
    """One layer at (n, cin, size, size) -> cout; form: 'plain' | 'stats' (store_n = n / 2) |
    'adain' (the AdaIN loader)."""
    g = torch.Generator(device=dev).manual_seed(cin * 1000 + cout)
    x = torch.rand((n, cin, size, size), device=dev, generator=g)
    w = (torch.rand((cout, cin, 3, 3), device=dev, generator=g) - 0.5) * (24.0 / (cin * 9)) ** 0.5
    b = (torch.rand((cout,), device=dev, generator=g) - 0.5) * 0.1
    p32, p16 = ops.pack_conv_weight(w), ops.pack_conv_weight_bf16(w)
    aux = None
    stored = n
    if form == "adain":
        st = [torch.rand((n, cin, 1, 1), device=dev, generator=g) * 0.5 + 0.5 for _ in range(4)]
        aux = ops.adain_params(*st)
    if form == "stats":
        stored = n // 2

        def f32():
            ops.conv2d_stats(x, p32, b, cout, 3, pad=ops.PAD_ZERO, relu=True, store_n=stored)

        def f16():
            ops.conv2d_bf16(x, p16, b, cout, pad=ops.PAD_ZERO, relu=True, stats=True,
                            store_n=stored)
    else:
        in_op = ops.IN_ADAIN if form == "adain" else ops.IN_NONE

        def f32():
            ops.conv2d(x, p32, b, cout, 3, pad=ops.PAD_ZERO, in_op=in_op, relu=True, aux=aux)

        def f16():
            ops.conv2d_bf16(x, p16, b, cout, pad=ops.PAD_ZERO, in_op=in_op, relu=True, aux=aux)
    t = interleaved({"fp32_a": f32, "bf16": f16, "fp32_b": f32}, rounds)
    flop = 2.0 * n * cout * cin * 9 * size * size
    nbytes = 4.0 * size * size * (n * cin + stored * cout)
    ms = t["bf16"]["ms"]
    algo = ops._ALGO_TAG[ops.conv_algorithm(cout, cin, size, size, 3, in_op if form != "stats"
                                            else ops.IN_NONE)]
    return {"layer": f"{cin}->{cout}", "form": form, "n": n, "size": size, "fp32_kernel": algo,
            "kept": ops.conv2d_bf16_supports(cout, cin, 3, ops.PAD_ZERO,
                                             ops.IN_ADAIN if form == "adain" else ops.IN_NONE),
            **t, "fp32_spread_ms": round(abs(t["fp32_a"]["ms"] - t["fp32_b"]["ms"]), 4),
            "bf16_over_fp32": round(ms / min(t["fp32_a"]["ms"], t["fp32_b"]["ms"]), 4),
            "bf16_tflops": round(flop / ms / 1e9, 1),
            "bf16_mfma_peak_share": round(flop / ms / 1e9 / PEAK_BF16_TFLOPS, 4),
            "bf16_gbps": round(nbytes / ms / 1e6, 1),
            "bf16_hbm_peak_share": round(nbytes / ms / 1e6 / PEAK_HBM_GBPS, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=32, help="content images (as many style images)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16", "bench_bf16.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bf16: needs a ROCm GPU")
    import network as net
    from rpst import ops, synth
    dev = torch.device("cuda:0")
    n, size, hd = args.n, args.size, args.hidden
    result = {"n": n, "size": size, "hidden_dim": hd, "rounds": args.rounds, "layers": []}
    if not args.skip_layers:
        enc = [(hd * 2 ** i, hd * 2 ** (i + 1)) for i in range(4)]
        layers = [(2 * n, ci, co, "stats" if i == 3 else "plain") for i, (ci, co) in enumerate(enc)]
        layers += [(n, co, ci, "adain" if i == 0 else "plain")
                   for i, (ci, co) in enumerate(reversed(enc))]
        for nn_, ci, co, form in layers:
            row = layer_row(ops, dev, nn_, ci, co, size, form, args.rounds)
            print(json.dumps(row), flush=True)
            result["layers"].append(row)
            torch.cuda.empty_cache()
    cfg = {"rp_blocks": 5, "hidden_dim": hd, "content_weight": 1.0, "style_weight": 10.0,
           "resume": False, "use_mask": False}
    model = net.AdaINRPNet(cfg, copy.deepcopy(net.vgg))
    synth.synth_module_(model, 0)
    model = model.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    content = torch.rand((n, 3, size, size), device=dev, generator=g)
    style = torch.rand((n, 3, size, size), device=dev, generator=g)

    def run(precision):
        def f():
            model.precision = precision
            model.test(content, style)
        return f

    t = interleaved({"fp32_a": run("fp32"), "bf16": run("bf16"), "fp32_b": run("fp32")},
                    args.rounds)
    model.precision = "fp32"
    y32 = model.test(content, style)
    model.precision = "bf16"
    y16 = model.test(content, style)
    rel = float((y16.double() - y32.double()).norm() / y32.double().norm())
    result["test"] = {**t, "fp32_spread_ms": round(abs(t["fp32_a"]["ms"] - t["fp32_b"]["ms"]), 4),
                      "bf16_over_fp32": round(t["bf16"]["ms"] / min(t["fp32_a"]["ms"],
                                                                    t["fp32_b"]["ms"]), 4),
                      "images_per_s_fp32": round(n / min(t["fp32_a"]["ms"], t["fp32_b"]["ms"]) * 1e3, 1),
                      "images_per_s_bf16": round(n / t["bf16"]["ms"] * 1e3, 1),
                      "rel_l2_bf16_vs_fp32": rel}
    print(json.dumps({"test": result["test"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

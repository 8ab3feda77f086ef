"""LDMSAdaINRPNet (`network: ld_adain`) training: the 7x7 backward kernels per layer and the
whole training step against torch autograd (one MI355X).

    python tools/bench_ld_train.py kernels [--n 8] [--size 512] [--rounds 3] [--out F.json]
    python tools/bench_ld_train.py step [--n 8 4 2] [--size 512] [--rounds 3] [--out F.json]

kernels: per 7x7 layer C -> C (32, 64, 128, 256) at (N, C, size, size), in one process,
alternating, after a warm-up; `rounds` windows (HIP events on the launch stream) of enough
calls to fill a second each, the median window per call with the windows' min / max:
  conv7     ops.conv2d_k7, reflect pad 3, LeakyReLU, bias (the forward)   FLOP = 2 C C 49 H W N
  wgrad7    autograd.conv_wgrad7, reflect pad 3, with the bias gradient    the same FLOP
  dgrad7    autograd.conv_dgrad of the reflect-padded conv: embed + rpst_conv7 over
            (H+6) x (W+6) + rpst_reflect_pad_backward                      the same FLOP (nominal)
  fold      rpst_reflect_pad_backward alone (no FLOP; GB/s of its bytes)
TF/s are the nominal FLOP over the median, `frac` their share of the 157.3 TF/s fp32 MFMA peak:
a kernel's share of peak, not a step rate.

step: hidden_dim 16, ld_layer_num 5, synthetic weights, N content / style pairs at size^2: one
training step = ld_losses + backward (gradients of every rp_enc* / rp_dec* parameter; no
optimizer) on the kernels, next to torch autograd of the same network restated from plain
torch.nn layers in fp32 on the same GPU (a deep copy's own layers: ReflectionPad2d + Conv2d +
LeakyReLU blocks, torch AdaIN, torch VGG losses), run alternately, one step per window (a step
is over a second at these sizes), `rounds` windows each after a warm-up step (whose wall time
is printed: torch's first step includes MIOpen's search per conv shape; MIOPEN_FIND_MODE is
recorded). Whole-step rate:
images/s = N / median. --n takes candidates in order; the first whose two steps both fit in
memory is measured and stated, with both sides' peak allocated bytes."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rp-style-transfer_amd"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_TFLOPS = 157.3
CHANNELS = (32, 64, 128, 256)
CONFIG = {"rp_blocks": 5, "hidden_dim": 16, "content_weight": 1.0, "style_weight": 10.0,
          "resume": False, "use_mask": False, "shuffle": False, "shuffle_layers": 1,
          "sort": False, "stylized_layers": 5, "enc_stack_way": "NONE", "inception_num": 0,
          "attention": "none", "ld_layer_num": 5}


def window(fn, reps):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def medians(fns, rounds, target_ms=1000.0):
    """name -> (median, min, max, reps) ms per call over `rounds` windows, alternating."""
    reps = {}
    for k, fn in fns.items():  # warm-up: code objects, allocator
        fn()
        reps[k] = max(1, min(500, int(target_ms / max(window(fn, 1), 1e-3)) + 1))
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, reps[k]))
    return {k: (statistics.median(v), min(v), max(v), reps[k]) for k, v in times.items()}


def bench_kernels(args):
    from rpst import _lib, ops, plan
    from rpst import autograd as A
    dev = torch.device("cuda:0")
    n, hw = args.n[0], args.size
    rows = []
    for c in args.channels:
        g = torch.Generator(device=dev).manual_seed(c)
        x = torch.rand((n, c, hw, hw), device=dev, generator=g) - 0.5
        dy = torch.rand((n, c, hw, hw), device=dev, generator=g) - 0.5
        conv = nn.Conv2d(c, c, 7).to(dev)
        with torch.no_grad():
            conv.weight.copy_((torch.rand((c, c, 7, 7), device=dev, generator=g) - 0.5)
                              * (12.0 / (c * 49)) ** 0.5)
        step = plan.ConvStep(conv=conv, pad=ops.PAD_REFLECT, in_op=ops.IN_NONE,
                             relu=ops.ACT_LRELU)
        out = torch.empty_like(x)
        gp = torch.rand((n, c, hw + 6, hw + 6), device=dev, generator=g) - 0.5

        def conv7():
            plan.conv(step, x, out=out)

        def wgrad7():
            A.conv_wgrad7(x, dy, conv, ops.PAD_REFLECT)

        def dgrad7():
            A.conv_dgrad(dy, step)

        def fold():
            _lib.call("rpst_reflect_pad_backward", gp.data_ptr(), out.data_ptr(), n * c, hw, hw,
                      3, ops._stream(gp))

        with torch.no_grad():
            res = medians({"conv7": conv7, "wgrad7": wgrad7, "dgrad7": dgrad7, "fold": fold},
                          args.rounds)
        flop = 2.0 * c * c * 49 * hw * hw * n
        for k, (med, lo, hi, reps) in res.items():
            r = {"op": k, "shape": [n, c, hw, hw], "ms": round(med, 4), "ms_min": round(lo, 4),
                 "ms_max": round(hi, 4), "reps": reps, "rounds": args.rounds}
            if k == "fold":
                r["GBps"] = round(4.0 * (gp.numel() + out.numel()) / med / 1e6, 1)
            else:
                tf = flop / med / 1e9
                r.update({"TFps": round(tf, 2), "frac_of_157.3": round(tf / PEAK_TFLOPS, 4),
                          "x_forward": round(med / res["conv7"][0], 3)})
            print(json.dumps(r), flush=True)
            rows.append(r)
        del x, dy, out, gp, conv, step
        torch.cuda.empty_cache()
    return rows


# ---- the torch baseline ---------------------------------------------------------------------
def _mean_std(x, eps=1e-5):
    n, c = x.shape[:2]
    v = x.reshape(n, c, -1)
    return v.mean(dim=2).view(n, c, 1, 1), (v.var(dim=2) + eps).sqrt().view(n, c, 1, 1)


def _adain(a, b):
    ma, sa = _mean_std(a)
    mb, sb = _mean_std(b)
    return (a - ma) / sa * sb + mb


class TorchLD(nn.Module):
    """The network's loss graph from plain torch.nn layers (a deep copy's own pads, convs and
    activations in nn.Sequential), the reference's op order: the encoder over content and over
    style, decode, VGG style / content losses."""

    def __init__(self, model):
        super().__init__()
        from rpst import plan
        m = copy.deepcopy(model)
        self.L = m.layer_num
        self.cw, self.sw = float(m.config["content_weight"]), float(m.config["style_weight"])
        seq = lambda blk: nn.Sequential(*plan.block_layers(blk))  # noqa: E731
        self.small = nn.ModuleList(seq(m._enc(i, "small")) for i in range(self.L))
        self.big = nn.ModuleList(seq(m._enc(i, "big")) for i in range(self.L))
        self.dec = nn.ModuleList(seq(getattr(m, f"rp_dec{i}")) for i in range(self.L))
        self.vgg = nn.ModuleList(nn.Sequential(*getattr(m, f"enc_{i + 1}").children())
                                 for i in range(4))
        for p in self.vgg.parameters():
            p.requires_grad = False

    def levels(self, x):
        feats = []
        for i in range(self.L):
            x = torch.cat([self.small[i](x), self.big[i](x)], dim=1)
            feats.append(x)
        return feats

    def vgg_feats(self, x):
        out = []
        for enc in self.vgg:
            x = enc(x)
            out.append(x)
        return out

    def forward(self, content, style):
        cfs, sfs = self.levels(content), self.levels(style)
        y = self.dec[0](_adain(cfs[-1], sfs[-1]))
        for j, sf in enumerate(sfs[:-1][::-1]):
            y = self.dec[j + 1](y + _adain(y, sf))
        with torch.no_grad():
            ts, tc = self.vgg_feats(style), self.vgg_feats(content)[-1]
        fy = self.vgg_feats(y)
        ls = 0.0
        for a, b in zip(fy, ts):
            (ma, sa), (mb, sb) = _mean_std(a), _mean_std(b)
            ls = ls + F.mse_loss(ma, mb) + F.mse_loss(sa, sb)
        lc = F.mse_loss(fy[-1], tc)
        return self.cw * lc + self.sw * ls


def bench_step(args):
    import network as net
    from rpst import autograd as A
    from rpst import synth
    dev = torch.device("cuda:0")
    m = net.LDMSAdaINRPNet(CONFIG, copy.deepcopy(net.vgg))
    synth.synth_module_(m, 3)
    m = m.to(dev)
    tm = None if args.no_torch else TorchLD(m).to(dev)
    total_mem = torch.cuda.get_device_properties(dev).total_memory

    def ours(c, s):
        m.zero_grad(set_to_none=True)
        _, total = A.ld_losses(m, c, s)
        total.backward()
        return total.detach()

    def theirs(c, s):
        tm.zero_grad(set_to_none=True)
        total = tm(c, s)
        total.backward()
        return total.detach()

    def ours_f4(c, s):
        os.environ["RPST_TRAIN_F4"] = "ld"  # read by ops.precise_convs at every step
        try:
            return ours(c, s)
        finally:
            del os.environ["RPST_TRAIN_F4"]

    sides = (("rpst", ours),)
    if args.forms:
        sides += (("rpst_f4", ours_f4),)
    if tm is not None:
        sides += (("torch", theirs),)
    for n in args.n:
        shape = (n, 3, args.size, args.size)
        c = torch.from_numpy(synth.image(1, shape)).to(dev)
        s = torch.from_numpy(synth.image(2, shape)).to(dev)
        peaks, totals = {}, {}
        try:
            for name, fn in sides:  # warm-up, and does it fit
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.time()
                totals[name] = float(fn(c, s))
                torch.cuda.synchronize()
                peaks[name] = torch.cuda.max_memory_allocated()
                print(json.dumps({"n": n, "warm_up": name, "seconds": round(time.time() - t0, 1),
                                  "peak_allocated_bytes": peaks[name]}), flush=True)
        except torch.cuda.OutOfMemoryError:
            print(json.dumps({"n": n, "fits": False}), flush=True)
            m.zero_grad(set_to_none=True)
            if tm is not None:
                tm.zero_grad(set_to_none=True)
            del c, s
            torch.cuda.empty_cache()
            continue
        times = {name: [] for name, _ in sides}
        for _ in range(args.rounds):
            for name, fn in sides:
                times[name].append(window(lambda: fn(c, s), 1))
        row = {"op": "LD training step (forward + backward)", "hidden": 16, "layers": 5,
               "shape": list(shape), "rounds": args.rounds, "device_bytes": total_mem,
               "miopen_find_mode": os.environ.get("MIOPEN_FIND_MODE", "default"),
               "total_loss": totals}
        if tm is not None:  # the two sides computed the same step
            row["first_block_grad_rel_l2_vs_torch"] = max(
                float((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-30))
                for (_, p), (_, q) in zip(
                    sorted((k, p) for k, p in m.named_parameters()
                           if k.startswith("rp_enc0_small")),
                    sorted((k, p) for k, p in tm.small[0].named_parameters())))
        for name, v in times.items():
            med = statistics.median(v)
            row[name] = {"ms": round(med, 2), "ms_min": round(min(v), 2),
                         "ms_max": round(max(v), 2), "img_per_s": round(n / med * 1e3, 3),
                         "windows_ms": [round(t, 2) for t in v],
                         "peak_allocated_bytes": peaks[name]}
        if tm is not None:
            row["speedup_median"] = round(statistics.median(times["torch"])
                                          / statistics.median(times["rpst"]), 3)
            row["speedup_worst_case"] = round(min(times["torch"]) / max(times["rpst"]), 3)
        print(json.dumps(row), flush=True)
        return [row]
    raise SystemExit("bench_ld_train: no candidate batch fits")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", choices=["kernels", "step"])
    ap.add_argument("--n", type=int, nargs="+", default=[8])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    ap.add_argument("--no-torch", action="store_true",
                    help="step: without the torch baseline")
    ap.add_argument("--forms", action="store_true",
                    help="step: also the kernels' step with RPST_TRAIN_F4=ld (F(4x4) on the 3x3 "
                         "chains), alternating with the default precise form")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ld_train: needs a ROCm GPU")
    rows = bench_kernels(args) if args.mode == "kernels" else bench_step(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

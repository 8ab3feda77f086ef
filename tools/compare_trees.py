"""Bit-for-bit comparison of two trees of this repository on the GPU.

    python tools/compare_trees.py PARENT_ROOT NEW_ROOT [--cases a,b,..] [--work DIR] [--log FILE]

PARENT_ROOT is a checkout of the parent commit (`git archive <commit> | tar -x -C DIR`) with its
own built librpst.so, NEW_ROOT this tree. Every case (CASES) runs once per tree, the parent
first, in a fresh child process started with subprocess under its own timeout, one GPU process
at a time; the first non-zero exit stops the run. The child wraps rpst._lib.call to log each
entry point's name and its non-pointer arguments (a pointer is logged as null / non-null),
runs the case under ops.TRACE on seeded inputs and saves, with torch.save, the output tensors
(test() outputs, or losses and every parameter gradient), the call log and TRACE.summary().
A case passes when the tensors are torch.equal, the call logs are identical and the trace
summaries have the same keys, launches, FLOPs and bytes. The ops.* cases build no model: they run
one rpst.ops function on seeded features at each listed shape and save every output. COVERAGE lists the entry points the
parent's logs must reach over all cases. Reads nothing outside the two trees; exit status 0
only if every case passes and the coverage is complete.
"""
from __future__ import annotations

import argparse
import copy
import os
import subprocess
import sys

COVERAGE = """rpst_conv2d rpst_conv2d_ws rpst_conv2d_pair rpst_conv2d_pool rpst_conv2d_masked
rpst_conv2d_skip_adain rpst_conv2d_stats rpst_conv2d_stats_store rpst_conv2d_mix rpst_conv2d_gated
rpst_conv7 rpst_maxpool2x2_ceil rpst_upsample_nearest2x rpst_conv_wgrad_pad rpst_conv7_wgrad
rpst_conv1x1_wgrad rpst_reflect_pad_border_grad_masked rpst_reflect_pad_backward rpst_wct_fuse
rpst_wct_params rpst_whiten_and_color_f64 rpst_whiten_and_color_original_f64
rpst_matrix_power_psd_f64 rpst_adain rpst_mean_variance_norm rpst_masked_adain_params
rpst_resized_mean_std rpst_sanet_attention rpst_cosine_affinity rpst_aea_clamp
rpst_adaptive_attention rpst_sanet_attention_backward rpst_sanet_attention_backward_chunked
rpst_adaptive_attention_backward rpst_adain_backward rpst_sq_diff_sum""".split()

RP = {"rp_blocks": 5, "hidden_dim": 16, "content_weight": 1.0, "style_weight": 10.0,
      "resume": False, "use_mask": False}
MS = dict(RP, shuffle=False, shuffle_layers=1, sort=False, stylized_layers=5,
          enc_stack_way="constant", inception_num=0, attention="none")
LD = dict(MS, rp_blocks=3, stylized_layers=3, ld_layer_num=3, enc_stack_way="NONE")
SA = {"content_weight": 1.0, "style_weight": 3.0, "l_identity1_weight": 50.0,
      "l_identity2_weight": 1.0}
SOURCE = {"use_mask": False, "content_weight": 1.0, "style_weight": 10.0}

# case -> (model class, (config, arguments after the VGG..), what runs, environment);
# what: "test", "test_mask" (label maps at feat x feat), "forward_nograd", an rpst.autograd entry,
# or "ops:<name>": no model, OPS[name] on each item of the arguments (the smallest shapes that
# reach each branch of the WCT entry points)
CASES = {
    "adain.test": ("AdaINRPNet", (RP,), "test", {}),
    "adain.test.unfused": ("AdaINRPNet", (RP,), "test", {"RPST_FUSE_ADAIN": "0"}),
    "adain.forward_nograd": ("AdaINRPNet", (RP,), "forward_nograd", {}),
    "wct.test": ("WCTRPNet", (RP,), "test", {"RPST_FUSE_WCT": "1"}),
    "wct.test.unfused": ("WCTRPNet", (RP,), "test", {"RPST_FUSE_WCT": "0"}),
    "samodel.test": ("SAModel", (SA, 0, 64), "test", {}),
    "adaptive.test": ("AdaptiveSAModel", (dict(SA, ada_module="relu"), 0, 64), "test", {}),
    "source.test": ("SourceNet", (SOURCE,), "test", {}),
    # the one case added for COVERAGE: at these shapes only the separate pool pass (the
    # RPST_POOL_EPILOGUE=0 route of plan.lower) reaches rpst_maxpool2x2_ceil
    "source.test.pool_pass": ("SourceNet", (SOURCE,), "test", {"RPST_POOL_EPILOGUE": "0"}),
    "source.test.mask": ("SourceNet", (dict(SOURCE, use_mask=True),), "test_mask:8", {}),
    "multiscale.test": ("MultiScaleAdaINRPNet", (MS,), "test", {}),
    "multiscale.test.deeper": ("MultiScaleAdaINRPNet",
                               (dict(MS, enc_stack_way="deeper", inception_num=3),), "test", {}),
    "multiscale.test.se": ("MultiScaleAdaINRPNet", (dict(MS, attention="se"),), "test", {}),
    "multiscale.test.mask": ("MultiScaleAdaINRPNet", (dict(MS, use_mask=True),), "test_mask:64",
                             {}),
    "ld.test": ("LDMSAdaINRPNet", (LD,), "test", {}),
    "ld4.test": ("LDMSAdaINRPNet4", (LD,), "test", {}),
    "ld.test.inception1": ("LDMSAdaINRPNet", (dict(LD, inception_num=1),), "test", {}),
    "adain.losses": ("AdaINRPNet", (RP,), "adain_rp_losses", {}),
    "wct.losses": ("WCTRPNet", (RP,), "wct_rp_losses", {}),
    "samodel.losses": ("SAModel", (SA, 0, 64), "samodel_losses", {}),
    "adaptive.losses": ("AdaptiveSAModel", (dict(SA, ada_module="relu"), 0, 64),
                        "samodel_losses", {}),
    "source.losses": ("SourceNet", (SOURCE,), "sourcenet_losses", {}),
    "multiscale.losses": ("MultiScaleAdaINRPNet", (MS,), "multiscale_losses", {}),
    "ld.losses": ("LDMSAdaINRPNet", (LD,), "ld_losses", {}),
    # (n, C, h, w): NB 4 scalar loads | scalar | NB 8 16-B loads | 16-wave | 16-wave, C % 16 != 0,
    # scalar | tiled SYRK, 128 tiles, one partial | tiled, scalar | HW = 8192: two K splits
    "ops.wct_fuse": (None, ((3, 16, 5, 7), (1, 64, 33, 31), (2, 128, 16, 24), (2, 256, 16, 16),
                            (1, 200, 9, 13), (1, 320, 16, 16), (1, 272, 9, 13),
                            (1, 320, 64, 128)), "ops:wct_fuse", {}),
    "ops.wct_fuse.t_f64": (None, ((2, 128, 16, 24),), "ops:wct_fuse", {"RPST_WCT_T_F64": "1"}),
    # (n, C, h, w, means given): the last one widens the means for the tiled SYRK
    "ops.wct_params": (None, ((2, 64, 24, 40, False), (2, 64, 24, 40, True),
                              (1, 320, 16, 16, True)), "ops:wct_params", {}),
    # (method, C, HW): 64 tiles scalar | 128 tiles, one partial | two K splits | Li et al.
    "ops.whiten_and_color": (None, (("closed-form", 64, 1023), ("closed-form", 160, 352),
                                    ("closed-form", 64, 8192), ("original", 64, 352)),
                             "ops:whiten_and_color", {}),
    # a PSD batch (Newton-Schulz) and one indefinite symmetric matrix (the Jacobi route)
    "ops.matrix_power_psd": (None, (("psd", 3, 96), ("indefinite", 1, 40)),
                             "ops:matrix_power_psd", {}),
    # (n, Cin, h, w, Cout): T x + c materialised (wct_apply_f32) | folded into the weights
    "ops.conv2d_mix": (None, ((2, 8, 9, 13, 32), (1, 16, 12, 20, 32)), "ops:conv2d_mix", {}),
    # the workspace layouts no model case reaches, at the smallest shapes that reach each branch
    # (mode, B, HW, hidden): AEAModule | AEALReluModule
    "ops.aea_clamp": (None, ((0, 2, 48, 16), (1, 2, 48, 16)), "ops:aea_clamp", {}),
    "ops.cosine_affinity": (None, ((2, 24, 6, 8),), "ops:cosine_affinity", {}),
    # C = 24: the two-GEMM path with S in the workspace
    "ops.sanet_attention": (None, ((2, 24, 6, 8),), "ops:sanet_attention", {}),
    # (B, C, h, w, mode, claim maps kept): two-GEMM path | flash path (C = 64, HW = 64)
    "ops.adaptive_attention": (None, ((2, 24, 6, 8, 0, False), (2, 24, 6, 8, 1, True),
                                      (2, 64, 8, 8, 1, False), (2, 64, 8, 8, 0, True)),
                               "ops:adaptive_attention", {}),
    # (entry, B, C, HWc, HWs[, hidden, mode]): the single pass | HW = 2304: two query chunks
    "ops.attention_backward": (None, (("sanet_attention_backward", 2, 64, 48, 40),
                                      ("sanet_attention_backward_chunked", 1, 64, 2304, 40),
                                      ("adaptive_attention_backward", 1, 24, 2304, 2304, 8, 1)),
                               "ops:attention_backward", {}),
    "ops.adain": (None, ((2, 24, 6, 8),), "ops:adain", {}),
}
SHAPE = (2, 3, 64, 64)


def features(seed: int, n: int, C: int, hw: int, dead=None):
    """(n, C, hw) fp64 conditioned features, one seed per image; channel `dead` zeroed."""
    import numpy as np
    import torch
    from rpst import synth
    x = np.stack([synth.conditioned_features(seed + i, C, hw) for i in range(n)])
    if dead is not None:
        x[:, dead] = 0.0
    return torch.from_numpy(x)


def run_ops(name: str, items, dev) -> dict:
    """Every output of rpst.ops.<name> on each item's seeded inputs (one dead style channel)."""
    import torch
    from rpst import ops, synth
    out = {}

    def pair(n, C, h, w):
        return (features(10, n, C, h * w).float().reshape(n, C, h, w).to(dev),
                features(20, n, C, h * w, dead=3).float().reshape(n, C, h, w).to(dev))

    def rnd(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)

    def f_psi(hw, hid):
        torch.manual_seed(70)
        return torch.nn.Sequential(torch.nn.Linear(hw, hid), torch.nn.LeakyReLU(0.2),
                                   torch.nn.Linear(hid, 1)).to(dev).requires_grad_(False)

    for item in items:
        if name == "aea_clamp":
            mode, B, hw, hid = item
            res = ops.aea_clamp(rnd(71, B, hw, hw).tanh(), rnd(72, B, hw, hw).softmax(-1),
                                f_psi(hw, hid), mode, 50.0, 0.0, 1.0)
            keys = ("clamp_fx", "clamp_value")
        elif name == "cosine_affinity":
            res = (ops.cosine_affinity(rnd(73, *item), rnd(74, *item)),)
            keys = ("affinity",)
        elif name == "sanet_attention":
            res = (ops.sanet_attention(rnd(75, *item), rnd(76, *item), rnd(77, *item)),)
            keys = ("out",)
        elif name == "adaptive_attention":
            B, C, h, w, mode, keep = item
            res = ops.adaptive_attention(*(rnd(80 + i, B, C, h, w) for i in range(5)),
                                         f_psi(h * w, 16), mode, 50.0, 0.0, 1.0, keep_claims=keep)
            res = tuple(r for r in res if r is not None)
            keys = ("out", "claim_value", "claim_before", "claim_after")
        elif name == "attention_backward":
            res = attention_backward(rnd, f_psi, *item)
            keys = ("dF", "dG", "dH", "dw1", "db1", "dw2", "db2")
        elif name == "adain":
            x, y = rnd(90, *item), rnd(91, *item)
            res = (ops.adaptive_instance_normalization(x, y), ops.mean_variance_norm(x))
            keys = ("adain", "mean_variance_norm")
        elif name == "wct_fuse":
            c, s = pair(*item)
            res = ops.wct_fuse(c, s, status=True) + ops.wct_params(c, s, status=True)
            keys = ("out", "status", "T", "offset", "residual", "params status")
        elif name == "wct_params":
            c, s = pair(*item[:4])
            means = torch.cat([c.double().mean((2, 3)), s.double().mean((2, 3))]).float()
            res = ops.wct_params(c, s, means if item[4] else None, status=True)
            keys = ("T", "offset", "residual", "status")
        elif name == "whiten_and_color":
            method, C, hw = item
            res = ops.whiten_and_color(features(30, 1, C, hw)[0].to(dev),
                                       features(40, 1, C, hw, dead=3)[0].to(dev), method, status=True)
            keys = ("out", "status")
        elif name == "matrix_power_psd":
            kind, batch, n = item
            x = features(50, batch, n, 2 * n)
            A = x @ x.transpose(1, 2) / (2 * n)
            if kind == "indefinite":  # symmetric, eigenvalues of both signs
                A = A - torch.eye(n, dtype=A.dtype) * A.diagonal(dim1=1, dim2=2).mean()
            else:  # well inside the Newton-Schulz route
                A = A + 0.01 * torch.eye(n, dtype=A.dtype)
            res = tuple(ops.matrix_power_psd(A.to(dev), p) for p in (0.5, -0.5))
            keys = ("sqrt", "inv_sqrt")
        elif name == "conv2d_mix":
            n, cin, h, w, cout = item
            x, s = pair(n, cin, h, w)
            T, c, _ = ops.wct_params(x, s)
            wgt = torch.from_numpy(synth.conv_param(60, "mix.weight", (cout, cin, 3, 3))).to(dev)
            bias = torch.from_numpy(synth.conv_param(60, "mix.bias", (cout,))).to(dev)
            res = (T, c, ops.conv2d_mix(x, T, c, ops.pack_conv_weight(wgt), bias, cout, 3))
            keys = ("T", "offset", "out")
        else:
            raise KeyError(name)
        out.update({f"{item} {k}": v for k, v in zip(keys, res)})
    return out


def attention_backward(rnd, f_psi, entry, B, C, hwc, hws, hid=0, mode=0):
    """One attention backward entry point, called as rpst.autograd calls it, on seeded features
    (no autograd function reaches the single pass or two query chunks at the model cases'
    sizes) -> (dF, dG, dH[, dw1, db1, dw2, db2])."""
    import torch
    from rpst import _lib, ops
    F, dO = rnd(92, B, C, hwc), rnd(93, B, C, hwc)
    G, H = rnd(94, B, C, hws), rnd(95, B, C, hws)
    out = [torch.empty_like(t) for t in (F, G, H)]
    size = getattr(_lib.load(), f"rpst_{entry}_workspace_size")
    if entry == "adaptive_attention_backward":
        c, s = rnd(96, B, C, hwc), rnd(97, B, C, hws)
        w1, b1, w2, b2, _ = ops._mlp_params(f_psi(hwc, hid))
        out += [torch.empty_like(t) for t in (w1, b1, w2, b2)]
        nbytes = size(B, C, hwc, hid)
        args = ([t.data_ptr() for t in (F, G, H, c, s, w1, b1, w2, b2)] +
                [hid, mode, 50.0, 0.0, 1.0, dO.data_ptr()] + [t.data_ptr() for t in out] +
                [B, C, hwc])
    else:
        nbytes = size(B, hwc, hws) if entry == "sanet_attention_backward" else size(B, C, hwc, hws)
        args = ([t.data_ptr() for t in (F, G, H, dO)] + [t.data_ptr() for t in out] +
                [B, C, hwc, hws])
    ws = torch.empty(nbytes, device=F.device, dtype=torch.uint8)
    _lib.call(f"rpst_{entry}", *args, ws.data_ptr(), nbytes, ops._stream(F))
    return tuple(out)


def child(root: str, case: str, out_path: str) -> None:
    """Run one case on the tree at `root` and save what the parent process compares."""
    sys.path[:0] = [root, os.path.join(root, "rp-style-transfer_amd")]
    import torch

    import network as net
    from rpst import _lib, autograd, ops, synth

    assert os.path.realpath(_lib.LIB_PATH).startswith(os.path.realpath(root)), _lib.LIB_PATH
    cls, args, what, _ = CASES[case]
    dev = torch.device("cuda:0")
    if cls is not None:
        model = getattr(net, cls)(*copy.deepcopy(args[:1]), copy.deepcopy(net.vgg), *args[1:])
        synth.synth_module_(model, 7)
        model = model.to(dev)
    c = torch.from_numpy(synth.image(1, SHAPE)).to(dev)
    s = torch.from_numpy(synth.image(2, SHAPE)).to(dev)

    calls, real_call = [], _lib.call

    def logged_call(name, *a):
        types = _lib.SIGNATURES[name][1]
        calls.append((name, tuple(("null" if v is None else "ptr") if t is _lib._P else v
                                  for v, t in zip(a, types))))
        return real_call(name, *a)

    _lib.call = logged_call
    ops.TRACE = ops.Trace()
    tensors = {}
    if what.startswith("ops:"):
        tensors.update(run_ops(what[4:], args, dev))
    elif what == "test":
        tensors["out"] = model.test(c, s)
    elif what.startswith("test_mask"):
        side = int(what.split(":")[1])
        gen = torch.Generator().manual_seed(3)
        segs = [torch.randint(0, 4, (SHAPE[0], side, side), generator=gen).to(torch.uint8).to(dev)
                for _ in range(2)]
        tensors["out"] = model.test(c, s, c_mask_path=segs[0], s_mask_path=segs[1])
    elif what == "forward_nograd":
        with torch.no_grad():
            losses, _ = model(c, s)
        tensors.update(losses)
    else:
        losses, total = getattr(autograd, what)(model, c, s)
        total.backward()
        tensors.update(losses)
        tensors.update({"grad " + k: p.grad for k, p in model.named_parameters()
                        if p.grad is not None})
    torch.cuda.synchronize()
    trace = {k: (v["launches"], v["flops"], v["bytes"]) for k, v in ops.TRACE.summary().items()}
    torch.save({"tensors": {k: v.detach().cpu() for k, v in tensors.items()}, "calls": calls,
                "trace": trace}, out_path)


def compare(case: str, a: dict, b: dict, say) -> bool:
    import torch
    ta, tb = a["tensors"], b["tensors"]
    equal = [k for k in ta if k in tb and ta[k].shape == tb[k].shape and torch.equal(ta[k], tb[k])]
    grads = sum(k.startswith("grad ") for k in ta)
    ok_t = list(ta) == list(tb) and len(equal) == len(ta)
    say(f"{case}: {len(equal) - grads}/{len(ta) - grads} output / loss tensors, {grads} gradient "
        f"tensors torch.equal: {'ALL EQUAL' if ok_t else 'DIFFERENT'}")
    for k in ta:
        if k not in equal:
            say(f"   differs: {k}")
    ok_c = a["calls"] == b["calls"]
    say(f"   calls parent {len(a['calls'])}, new {len(b['calls'])}: "
        f"{'SAME SEQUENCE AND ARGUMENTS' if ok_c else 'DIFFERENT'}")
    if not ok_c:
        for i, (x, y) in enumerate(zip(a["calls"], b["calls"])):
            if x != y:
                say(f"   first difference at call {i}: parent {x} | new {y}")
                break
    ok_s = a["trace"] == b["trace"]
    say(f"   trace keys parent {len(a['trace'])}, new {len(b['trace'])}: "
        f"{'SAME KEYS, LAUNCHES, FLOPS, BYTES' if ok_s else 'DIFFERENT'}")
    if not ok_s:
        for k in sorted(set(a["trace"]) | set(b["trace"])):
            if a["trace"].get(k) != b["trace"].get(k):
                say(f"   {k}: parent {a['trace'].get(k)} | new {b['trace'].get(k)}")
    return ok_t and ok_c and ok_s


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--work", default="compare_trees_out", help="directory of the saved runs")
    ap.add_argument("--log", default=None, help="also append the report to this file")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", nargs=2, metavar=("CASE", "OUT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(os.path.abspath(a.new), *a.child)
        return 0
    import torch
    os.makedirs(a.work, exist_ok=True)
    log = open(a.log, "a") if a.log else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    say("# parent tree (git archive of the parent commit, its own librpst.so) vs this tree; one "
        "fresh process per case per tree, parent first;")
    say(f"# seeded inputs {SHAPE}; rpst_* calls logged with their non-pointer arguments by "
        "wrapping rpst._lib.call; tensors compared with torch.equal")
    say("# source.test.pool_pass (RPST_POOL_EPILOGUE=0) is the case added for coverage: no other "
        "case reaches rpst_maxpool2x2_ceil at these shapes")
    reached, ok = set(), True
    for case in a.cases.split(","):
        runs = []
        for tag, root in (("parent", os.path.abspath(a.parent)), ("new", os.path.abspath(a.new))):
            out = os.path.abspath(os.path.join(a.work, f"{case}.{tag}.pt"))
            env = dict(os.environ, **CASES[case][3])
            env.pop("RPST_LIB", None)  # each tree loads its own library
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__),
                   root, root, "--child", case, out]
            rc = subprocess.run(cmd, env=env, cwd=root).returncode
            if rc != 0:
                say(f"{case}: the {tag} tree's process exited with status {rc}: STOPPED")
                return 1
            runs.append(torch.load(out, weights_only=False))
        reached |= {name for name, _ in runs[0]["calls"]}
        ok &= compare(case, runs[0], runs[1], say)
    missing = [e for e in COVERAGE if e not in reached]
    say(f"# coverage of the parent's logs: {len(COVERAGE) - len(missing)}/{len(COVERAGE)} entry "
        f"points reached{': MISSING ' + ' '.join(missing) if missing else ''}")
    say(f"RESULT: {'PASS' if ok and not missing else 'FAIL'}")
    return 0 if ok and not missing else 1


if __name__ == "__main__":
    sys.exit(main())

"""Shared test helpers: tolerances, golden sets, the kernel tests' inputs, networks built from
golden cases, mask arguments, the fused / op-by-op switch, the launch spy, and the dataset
tree and shared body of the stylize pipeline tests."""
import contextlib
import os

import numpy as np
import torch

# Tolerances; measured fp32-vs-fp64 noise floor of the reference:
# AdaIN-RP rel-L2 1.8e-6, SANet 4.8e-6.
TOL_STATS = 1e-5       # stats / AdaIN, rel-L2
TOL_WCT = 1e-5         # WCT on the fp32 output, rel-L2
TOL_NET = 1e-4         # full networks in fp32, rel-L2
TOL_NET_MAXABS = 5e-4  # full networks: max-abs <= TOL_NET_MAXABS * max|ref|


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# A golden set is one <name>.npz, or, where that would pass 1 MiB (the size limit of a
# committed file), <name>.part00.npz, <name>.part01.npz, ...: each part holds at most
# GOLDEN_PART_BYTES of array data, and an array larger than GOLDEN_PIECE_BYTES is stored as
# consecutive pieces of its flattened data, "<key>::0", "<key>::1", ... beside "<key>::shape".
GOLDEN_PART_BYTES = 960 * 1024
GOLDEN_PIECE_BYTES = 480 * 1024


def save_golden(name, **arrays):
    """Write the golden set `name` (replacing its files); load_golden returns it unchanged."""
    import glob
    for old in glob.glob(os.path.join(GOLDEN_DIR, name + ".npz")) + glob.glob(
            os.path.join(GOLDEN_DIR, name + ".part[0-9][0-9].npz")):
        os.remove(old)
    entries = []
    for key, a in arrays.items():
        a = np.asarray(a)
        assert "::" not in key, key
        if a.nbytes <= GOLDEN_PIECE_BYTES:
            entries.append((key, a))
            continue
        flat = np.ascontiguousarray(a).reshape(-1)
        per = GOLDEN_PIECE_BYTES // a.itemsize
        entries.append((key + "::shape", np.array(a.shape, dtype=np.int64)))
        entries += [(f"{key}::{j}", flat[o:o + per])
                    for j, o in enumerate(range(0, flat.size, per))]
    if sum(a.nbytes for _, a in entries) <= GOLDEN_PART_BYTES:
        np.savez_compressed(os.path.join(GOLDEN_DIR, name + ".npz"), **dict(entries))
        return
    parts, size = [{}], 0
    for key, a in entries:
        if size + a.nbytes > GOLDEN_PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][key] = a
        size += a.nbytes
    for i, part in enumerate(parts):
        np.savez_compressed(os.path.join(GOLDEN_DIR, f"{name}.part{i:02d}.npz"), **part)


def load_golden(name):
    """The golden set `name` as a dict of arrays, whichever way it is stored."""
    import glob
    paths = sorted(glob.glob(os.path.join(GOLDEN_DIR, name + ".part[0-9][0-9].npz")))
    raw = {}
    for p in paths or [os.path.join(GOLDEN_DIR, name + ".npz")]:
        raw.update(np.load(p, allow_pickle=False))
    out = {}
    for key, a in raw.items():
        if "::" not in key:
            out[key] = a
        elif key.endswith("::shape"):
            base = key[:-len("::shape")]
            n = sum(1 for k in raw if k.startswith(base + "::")) - 1
            out[base] = np.concatenate([raw[f"{base}::{j}"] for j in range(n)]).reshape(a)
    return out


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def max_abs_ratio(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def synth_(model, seed):
    from rpst import synth
    synth.synth_module_(model, seed)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    return np.array(synth.checksum(sd))


def state_dict_of(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


# ---- inputs ---------------------------------------------------------------------------------
def gen(seed, shape, scale=1.0, offset=0.0, relu=False):
    """Uniform [-1, 1) values from torch's CPU generator, scaled and shifted (then clamped at 0
    with relu): the kernel tests' inputs."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 2 - 1) * scale + offset
    return x.clamp_min(0) if relu else x


def peaked_attention_inputs(B, C, h, w, seed):
    """(F, G), fp32 (B, C, h, w), with a live AEA clamp: every query has one dominant key (a
    random permutation per image) whose softmax probability is spread over about [0.3, 0.97],
    the range of the clamp values (aea: [0.4, 0.9]). G's key columns have unit length over C,
    F[b][:, q] = m G[b][:, perm[b][q]] + 0.05 noise with m = log(p / (1 - p) (HW - 1)): the
    dominant logit is ~m, the other HW - 1 are ~0. Drawn in float64 from torch's CPU generator
    in the order G, the permutations, p, the noise."""
    g = torch.Generator().manual_seed(seed)
    hw = h * w
    G = torch.randn((B, C, hw), generator=g, dtype=torch.float64)
    G = G / G.norm(dim=1, keepdim=True)
    perm = torch.stack([torch.randperm(hw, generator=g) for _ in range(B)])
    p = 0.3 + 0.67 * torch.rand((B, hw), generator=g, dtype=torch.float64)
    m = torch.log(p / (1 - p) * (hw - 1))
    noise = torch.randn((B, C, hw), generator=g, dtype=torch.float64)
    F = m[:, None, :] * torch.gather(G, 2, perm[:, None, :].expand(B, C, hw)) + 0.05 * noise
    return F.float().view(B, C, h, w), G.float().view(B, C, h, w)


def clamp_liveness(P, clamp, mode, scale=50.0):
    """Share of the query rows of P (B, HW, HW) on which the AEA clamp (B, HW, 1) is live:
    'aea': a key inside the sigmoid's unsaturated window, |scale (P - c)| < 4; 'relu': an
    active ReLU entry, P > c."""
    d = P.detach() - clamp.detach().view(P.shape[0], P.shape[1], 1)
    live = (scale * d).abs() < 4 if mode == "aea" else d > 0
    return float(live.any(-1).double().mean())


AEA_GRADS = ("dF", "dG", "dH", "f_psi.0.weight", "f_psi.0.bias", "f_psi.2.weight", "f_psi.2.bias")
_AEA_CASES = {}


class _ChainBmm(torch.autograd.Function):
    """bmm(A, B) with every element summed over k in order, one product at a time, in the
    operands' type: the order in which an MFMA tile accumulates (MFMA numerics),
    where a CPU sgemm blocks k. The backward is the plain bmm's."""

    @staticmethod
    def forward(ctx, A, B):
        ctx.save_for_backward(A, B)
        out = torch.zeros((A.shape[0], A.shape[1], B.shape[2]), dtype=A.dtype)
        for k in range(A.shape[2]):
            out.addcmul_(A[:, :, k:k + 1], B[:, k:k + 1, :])
        return out

    @staticmethod
    def backward(ctx, g):
        A, B = ctx.saved_tensors
        return torch.bmm(g, B.transpose(1, 2)), torch.bmm(A.transpose(1, 2), g)


def aea_attention_grads(F, G, H, c, s, dO, sd, mode, dtype, aea=None, chain=False):
    """Autograd in `dtype` on the CPU of O = H aea(A, softmax(F^T G))^T, sum(O dO) taken
    back: the oracle's restatement (oracle.restate.aea, or `aea` in its place) on (B, C, h, w)
    inputs and the module's state dict; with chain the logits F^T G are summed over the
    channels in order (_ChainBmm). Returns (O, clamp, P, Q, {name: gradient}) with the names
    of AEA_GRADS, all detached."""
    from oracle import restate as R
    B, C, h, w = F.shape
    Fd, Gd, Hd = (x.to(dtype).view(B, C, -1).clone().requires_grad_() for x in (F, G, H))
    sd = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in sd.items()}
    A = R.cal_affinity_matrix(c.to(dtype), s.to(dtype))
    P = torch.softmax((_ChainBmm.apply if chain else torch.bmm)(Fd.transpose(1, 2), Gd), -1)
    Q, clamp = (aea or R.aea)(A, P, sd, "", mode)
    O = torch.bmm(Hd, Q.transpose(1, 2))
    (O * dO.to(dtype).view(B, C, -1)).sum().backward()
    grads = dict(dF=Fd.grad.view(F.shape), dG=Gd.grad.view(F.shape), dH=Hd.grad.view(F.shape))
    grads.update({k: sd[k].grad for k in AEA_GRADS[3:]})
    return O.detach().view(F.shape), clamp.detach(), P.detach(), Q.detach(), grads


def aea_live_case(mode, shape, mod_seed=11):
    """The live-clamp case of the AEA backward tests at shape (B, C, h, w), formed once per
    session and shared (read only): F, G from peaked_attention_inputs (seed 3; seed 10 at
    C = 512, see aea_live_bars), H, c, s, dO from gen(23 .. 26), the module from
    synth_(mod_seed); the float64 reference and the bars of aea_live_bars, whose conditions
    are asserted."""
    import types

    import network as net
    key = (mode, tuple(shape), mod_seed)
    if key in _AEA_CASES:
        return _AEA_CASES[key]
    B, C, h, w = shape
    mod = (net.AEAModule if mode == "aea" else net.AEALReluModule)(h * w)
    synth_(mod, mod_seed)
    F, G = peaked_attention_inputs(B, C, h, w, 10 if C == 512 else 3)
    H, dO = gen(23, shape), gen(26, shape)
    c, s = gen(24, shape, 1.0, 0.2, relu=True), gen(25, shape, 1.0, 0.2, relu=True)
    args = (F, G, H, c, s, dO, state_dict_of(mod), mode)
    out, clamp, P, Q, g64 = aea_attention_grads(*args, torch.float64)
    bars = aea_live_bars(aea_fp32_forms(*args), g64, P, Q, clamp, mode)
    case = types.SimpleNamespace(mod=mod, F=F, G=G, H=H, c=c, s=s, dO=dO, out=out, clamp=clamp,
                                 P=P, Q=Q, g64=g64, bars=bars)
    _AEA_CASES[key] = case
    return case


def aea_fp32_forms(*args):
    """The oracle's own fp32 CPU autograd of aea_attention_grads(*args, ...) in two forms:
    as torch runs it, and with the logits summed over the channels in order (_ChainBmm)."""
    return [aea_attention_grads(*args, torch.float32, chain=chain)[4] for chain in (False, True)]


def aea_live_bars(g32s, g64, P, Q, clamp, mode):
    """Per-tensor bars max(1e-5, 3 x rel-L2(g32, g64)) of a live-clamp gradient check, from
    the oracle's own fp32 CPU autograd against its float64 one (the single-kernel base 1e-5,
    the factor 3 of grad_bar), g32 being the worse of the forms g32s (aea_fp32_forms), after
    the conditions that make the check mean something, all on the float64 reference: the clamp
    is live on at least 0.15 ('aea') / 0.30 ('relu') of the rows, 'aea' also has both saturated
    tails, no gradient is near zero (norm >= 1e-3) and no bar passes 1e-4.
    Why two forms: the slope-50 sigmoid and the cancelling sum of dc over the rows amplify the
    rounding of the logits, and the kernels' GEMM sums each logit as one k-ordered fp32 chain
    where the CPU's sgemm blocks k. At C = 512 the chain rounds 2 x worse (dF 1.2e-5 against
    6e-6), and the f_psi gradients of either form land anywhere in 1e-6 .. 7e-5 from one seed
    to the next (profiles/aea_live/stage_attribution.txt): a bar from the torch form alone is
    rounding luck. With the logits in chain order the CPU form reproduces the kernel's error
    to ~5 % at (1 | 2, 512, 32, 32), every other stage in fp32 moving the f_psi gradients
    by < 5e-6. Seed 10 is the first from 3 up at which both forms keep every bar of both
    C = 512 shapes and both modes under 1e-4 (3.5e-5; profiles/aea_live/seed_scan.txt); up to
    C = 64 the two forms agree."""
    live = clamp_liveness(P, clamp, mode)
    assert live >= (0.15 if mode == "aea" else 0.30), (mode, live)
    if mode == "aea":
        assert (Q > 0.9).any() and (Q < 1e-6).any()
    bars = {}
    for k, ref in g64.items():
        assert float(ref.norm()) >= 1e-3, (k, float(ref.norm()))
        bars[k] = max(1e-5, 3.0 * max(rel_l2(g32[k], ref) for g32 in g32s))
        assert bars[k] <= 1e-4, (k, bars[k])
    print(f"aea live {mode} {tuple(P.shape)}: liveness {live:.3f}, bars "
          + " ".join(f"{k} {v:.2e}" for k, v in bars.items()))
    return bars


def flat_or_live(cases):
    """(id, case) pairs x inputs in {flat, live} as pytest params (*case, inputs): the flat
    inputs are the nearly flat softmax the kernel tests had alone at first (the clamp is
    dead there) and keep the ids the cases had then, the live ones add '-live'."""
    import pytest
    return [pytest.param(*case, inputs, id=cid + ("-live" if inputs == "live" else ""))
            for inputs in ("flat", "live") for cid, case in cases]


def aea_backward_abi(mod, F, G, H, c, s, dO):
    """rpst_adaptive_attention_backward through the C ABI on GPU tensors of one shape
    (B, C, h, w) or (B, C, HW), with the workspace of its own size function (uninitialised):
    ({name: gradient} under the names of AEA_GRADS, the workspace's bytes). mod: the AEA
    module, on the GPU."""
    from rpst import _lib, ops
    B, C = F.shape[:2]
    hw = F[0, 0].numel()
    with torch.no_grad():
        w1, b1, w2, b2, hid = ops._mlp_params(mod.f_psi)
    nbytes = _lib.load().rpst_adaptive_attention_backward_workspace_size(B, C, hw, hid)
    ws = torch.empty(nbytes, device=F.device, dtype=torch.uint8)
    outs = [torch.empty_like(x) for x in (F, G, H, w1, b1, w2, b2)]
    _lib.call("rpst_adaptive_attention_backward", F.data_ptr(), G.data_ptr(), H.data_ptr(),
              c.data_ptr(), s.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
              b2.data_ptr(), hid, mod.mode, 50.0, 0.4, 0.5, dO.data_ptr(),
              *(x.data_ptr() for x in outs), B, C, hw, ws.data_ptr(), nbytes, ops._stream(F))
    return dict(zip(AEA_GRADS, outs)), nbytes


def check_aea_grads(got, g64, bars, what):
    """Every gradient of g64 within its bar in rel-L2, each figure printed first."""
    for k, ref in g64.items():
        e = rel_l2(got[k].view_as(ref), ref)
        print(f"{what} {k}: rel-L2 {e:.3e} (bar {bars[k]:.3e}, |ref| {float(ref.norm()):.3e})")
    for k, ref in g64.items():
        e = rel_l2(got[k].view_as(ref), ref)
        assert e < bars[k], (what, k, e, bars[k])


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dev(a, cuda):
    return t(a).to(cuda)


def use_conv_algo(monkeypatch, param, w4q=False):
    """The environment of one conv_algo fixture parameter: librpst reads RPST_CONV_ALGO per
    launch, and with w4q RPST_W4Q too ('winograd4_32' keeps every F(4x4) layer on the
    32-channel kernel, 'winograd4q' forces the position-quarter kernel, the rest run the
    production rule). Returns param."""
    monkeypatch.setenv("RPST_CONV_ALGO",
                       {"winograd4_32": "winograd4", "winograd4q": "winograd4"}.get(param, param))
    if w4q:
        monkeypatch.setenv("RPST_W4Q", {"winograd4_32": "0", "winograd4q": "2"}.get(param, "1"))
    return param


# ---- networks from golden cases -------------------------------------------------------------
def golden_net(cls, cfg, g, key, device=None, seed=None):
    """cls(cfg, a copy of the VGG) with the synthetic weights of the golden entry `key`
    (g[key + 'seed'], checked against g[key + 'checksum']), or of `seed` instead (then nothing
    is checked); moved to `device` when one is given."""
    import copy

    import network as net
    m = cls(cfg, copy.deepcopy(net.vgg))
    ck = synth_(m, int(g[key + "seed"]) if seed is None else seed)
    if seed is None:
        assert np.array_equal(ck, g[key + "checksum"]), key
    return m if device is None else m.to(device)


def check_net(y, ref, what):
    err, mx = rel_l2(y, ref), max_abs_ratio(y, ref)
    print(f"{what}: rel-L2 {err:.3e} max-abs {mx:.3e}")
    assert err < TOL_NET and mx < TOL_NET_MAXABS, (what, err, mx)


def mask_kw(g, key, cuda, tmp_path=None, mode="L", name="{tag}{b}.png"):
    """The test() mask arguments of the masked golden entry `key` ({} where g[key + 'use_mask']
    is recorded and False): the label maps as tensors at the image size (the reference's own
    resize of its files: g[key + 'cseg'] / 'sseg'), or, with tmp_path, the mask files
    themselves (g[key + 'cfile'] / 'sfile') written there in PNG mode `mode` under `name`."""
    if key + "use_mask" in g and not bool(g[key + "use_mask"]):
        return {}
    if tmp_path is None:
        return dict(c_mask_path=dev(g[key + "cseg"].astype(np.uint8), cuda),
                    s_mask_path=dev(g[key + "sseg"].astype(np.uint8), cuda))
    import masked_ref as M

    def paths(tag, files):
        return [M.write_mask_png(str(tmp_path / name.format(tag=tag, mode=mode, b=b)), files[b],
                                 mode) for b in range(files.shape[0])]
    return dict(c_mask_path=paths("c", g[key + "cfile"]), s_mask_path=paths("s", g[key + "sfile"]))


# ---- switches and spies ---------------------------------------------------------------------
@contextlib.contextmanager
def unfused(module, attr):
    """The op-by-op path: module.attr (FUSED_ADAIN, FUSED, FUSED_WCT) False inside the block,
    the value it had put back after."""
    was = getattr(module, attr)
    setattr(module, attr, False)
    try:
        yield
    finally:
        setattr(module, attr, was)


def traced_launches(fn):
    """Run fn() under rpst.ops.TRACE and a torch.cat spy -> (launch names, the operand shapes of
    every torch.cat call); both hooks are taken out again, also when fn raises."""
    from rpst import ops
    cats = []
    real_cat, was = torch.cat, ops.TRACE

    def spy(tensors, *a, **k):
        cats.append([tuple(x.shape) for x in tensors])
        return real_cat(tensors, *a, **k)

    ops.TRACE = ops.Trace()
    torch.cat = spy
    try:
        fn()
        names = [r[0] for r in ops.TRACE.records]
    finally:
        torch.cat = real_cat
        ops.TRACE = was
    return names, cats


# ---- the stylize pipeline -------------------------------------------------------------------
def dataset_tree(root, size, mask_size, modes, rng_seed, mask_seed0, masks=True):
    """Pairs content/in<k>.png, style/tar<k>.png (size x size, uniform bytes from
    default_rng(rng_seed), content before style) with labelme_segmentation/<stem>.png
    (blocks_mask seed mask_seed0 + k, PNG mode modes[k]); without masks both images of pair k
    are named p<k>.png and no mask is written."""
    from PIL import Image

    import masked_ref as M
    rng = np.random.default_rng(rng_seed)
    for d in ("content", "style") + (("labelme_segmentation",) if masks else ()):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for k, mode in enumerate(modes):
        for d, stem in (("content", f"in{k}"), ("style", f"tar{k}")):
            a = rng.integers(0, 256, size=(size, size, 3), dtype=np.uint8)
            Image.fromarray(a, "RGB").save(
                os.path.join(root, d, (stem if masks else f"p{k}") + ".png"))
            if masks:
                M.write_mask_png(os.path.join(root, "labelme_segmentation", stem + ".png"),
                                 M.blocks_mask(mask_size, mask_size, [0, 60, 120, 180],
                                               mask_seed0 + k), mode)


def check_pipeline(cfg, tmp_path, cuda, pairs=2):
    """stylize.main on cfg (plus output = tmp_path / 'out', written as YAML) with
    --synthetic-weights 5: every PNG it writes is the direct test() call's on the same pair
    through the pipeline's own uint8 conversion, beside a -cat.png. cfg holds test_dir,
    test_dataset, img_size and use_mask. Returns the rebuilt network and, per pair,
    (content, style, the uint8 image)."""
    import yaml
    from PIL import Image

    import stylize
    from rpst.imageio import DATASETS, load_image, to_tensor, to_uint8
    cfg = dict(cfg, output=str(tmp_path / "out"))
    cfg_path = str(tmp_path / "cfg.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    assert stylize.main(["--config", cfg_path, "--synthetic-weights", "5"]) == 0
    m = stylize.build_network(cfg, synthetic_seed=5).to(cuda)
    ds = DATASETS[cfg["test_dataset"]](cfg["test_dir"])
    assert len(ds) == pairs
    size = cfg["img_size"]
    out_dir = tmp_path / "out" / "test" / "test_output"
    items = []
    for i in range(len(ds)):
        cp, sp, cn, sn, cm, sm = ds.item(i)
        c = to_tensor(dev(load_image(cp, size)[None], cuda))
        s = to_tensor(dev(load_image(sp, size)[None], cuda))
        kw = dict(c_mask_path=[cm], s_mask_path=[sm]) if cfg["use_mask"] else {}
        ref = to_uint8(m.test(c, s, **kw))[0].cpu().numpy()
        got = np.asarray(Image.open(out_dir / f"{cn}-{sn}.png"))
        assert got.shape == (size, size, 3)
        assert np.array_equal(got, ref), (cn, sn)
        assert (out_dir / f"{cn}-{sn}-cat.png").exists()
        items.append((c, s, ref))
    return m, items


def rp_config(hidden, blocks=5):
    return {"rp_blocks": blocks, "hidden_dim": hidden, "content_weight": 1.0,
            "style_weight": 10.0, "resume": False, "use_mask": False}


def multiscale_config(hidden, blocks=5, inception=0):
    """MultiScaleAdaINRPNet config (config/rl/train_constant_multiscale_rp_adain_recon.yaml
    with hidden/blocks/inception varied)."""
    cfg = rp_config(hidden, blocks)
    cfg.update({"shuffle": False, "shuffle_layers": 1, "sort": False,
                "stylized_layers": blocks, "enc_stack_way": "constant",
                "inception_num": inception, "attention": "none"})
    return cfg


SOURCE_CONFIG = {"use_mask": False, "content_weight": 1.0, "style_weight": 10.0}


def deeper_config(hidden, blocks=5, inception=3):
    """MultiScaleAdaINRPNet 'deeper' stack (config/rl/train_deeper_multiscale_rp_adain.yaml:
    enc_stack_way deeper, inception_num 3, hidden 16)."""
    cfg = multiscale_config(hidden, blocks, inception)
    cfg["enc_stack_way"] = "deeper"
    return cfg


def ms_grads_config(g, i):
    """The MultiScaleAdaINRPNet config of case i of tests/golden/grads_ms.npz."""
    cfg = multiscale_config(int(g[f"hidden{i}"]), int(g[f"blocks{i}"]), int(g[f"inception{i}"]))
    cfg.update(enc_stack_way=str(g[f"way{i}"]), content_weight=float(g[f"cw{i}"]),
               style_weight=float(g[f"sw{i}"]))
    return cfg


def src_grads_config(g, i):
    """The SourceNet config of case i of tests/golden/grads_src.npz."""
    return dict(SOURCE_CONFIG, content_weight=float(g[f"cw{i}"]), style_weight=float(g[f"sw{i}"]))


def grad_probe(key, g):
    """(sum, sum of squares, dot with a fixed uniform probe) of one gradient tensor
    (tests/golden/gen_golden.gen_grads_sam stores these instead of ~8M SAModel gradients)."""
    from rpst import synth
    g = np.asarray(torch.as_tensor(g).detach().double().cpu(), dtype=np.float64).reshape(-1)
    pr = 2.0 * synth.uniform01(0, "gprobe:" + key, g.size) - 1.0
    return np.array([g.sum(), (g * g).sum(), (g * pr).sum()])


def probe_err(ours, ref, n):
    """Largest of the three probe differences, each scaled like a rel-L2 error by the
    reference gradient's norm (sum and probe dot: by norm * sqrt(n) and norm * sqrt(n/3))."""
    nrm = max(np.sqrt(ref[1]), 1e-300)
    return max(abs(ours[0] - ref[0]) / (nrm * np.sqrt(n)),
               abs(np.sqrt(max(ours[1], 0.0)) - nrm) / nrm,
               abs(ours[2] - ref[2]) / (nrm * np.sqrt(n / 3.0)))


TOL_GRAD = 1e-4  # training gradients: base bar per tensor / probe (rel-L2 scale)
GRAD_FLOOR_SAMPLES = 6  # fp32 rounding samples per golden case (gen_golden.gen_grad_floors)


def ulp_perturbed(x, seed):
    """x (fp32 numpy) with every element moved one fp32 ulp up or down at random: the same
    input to within fp32 resolution, a different rounding pattern downstream. Sample k >= 1
    of a gradient-golden case perturbs content / style with seeds 7000 + 2k / 7001 + 2k."""
    up = np.random.default_rng(seed).random(x.shape) < 0.5
    return np.where(up, np.nextafter(x, np.float32(np.inf)),
                    np.nextafter(x, np.float32(-np.inf))).astype(np.float32)
_FLOORS = None


def grad_bar(family, i, name, base=TOL_GRAD):
    """Bar of one training-gradient golden: max(base, 3 x the reference's own fp32 noise
    floor), the floor being the committed fp32 golden's distance to the same REFERENCE model
    re-run in float64 (tests/golden/grad_floors.npz, gen_golden.gen_grad_floors): a
    form as accurate as the reference's own fp32 passes whatever its rounding pattern."""
    global _FLOORS
    if _FLOORS is None:
        import os
        _FLOORS = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                            "golden", "grad_floors.npz")))
    return max(base, 3.0 * float(_FLOORS[f"{family}/{i}:{name}"]))


def check_grads_vs_fp64(family, i, named, g64, skip=()):
    """Training gradients `named` (name -> parameter with .grad, on the GPU) against float64
    gradients g64 of the oracle on the same weights and inputs: each g64 tensor is first
    pinned to the REFERENCE's float64 gradient (its probe in grad_floors.npz, to 1e-9), then
    every gradient tensor is held to grad_bar in full-tensor rel-L2. Returns the worst
    err / bar (x 1e-4)."""
    global _FLOORS
    grad_bar(family, i, next(iter(g64)))  # loads _FLOORS
    worst = 0.0
    for name, ref in g64.items():
        if name in skip:
            continue
        pin = probe_err(grad_probe(name, ref), _FLOORS[f"{family}/{i}/p64:{name}"], ref.numel())
        assert pin < 1e-9, (family, i, name, "oracle float64 off the reference's", pin)
        e = rel_l2(named[name].grad, ref)
        bar = grad_bar(family, i, name)
        worst = max(worst, e / bar * 1e-4)
        assert e < bar, (family, i, name, e, bar)
    return worst


def check_grads_rms_vs_fp64(family, i, content, style, step, oracle64, skip=(), oracle32=None):
    """The same, with both sides' rounding sampled like the floor: over the
    GRAD_FLOOR_SAMPLES inputs of the floor (the golden's, then ulp_perturbed copies), the RMS
    of every gradient tensor's rel-L2 to float64 (oracle64(content, style) -> {name: grad},
    pinned to the reference's at sample 0) is held to max(1e-4, 3 x the reference's fp32
    RMS). For the attention models, whose softmax-side gradients amplify the frozen VGG
    features' rounding ~1e3 x, one sample of either side is rounding luck. oracle32: the
    reference's algorithm (the oracle, bit-identical to the reference on the CPU) run in fp32
    on the GPU's own torch backend, as the reference trains: its RMS distance to float64 is a
    second measurement of the reference's fp32 noise on the same samples, and the floor is
    the larger of the two (the committed CPU one, grad_floors.npz). step(content, style) runs
    the kernels' training step and returns {name: parameter with .grad}. Returns the worst
    RMS / bar (x 1e-4)."""
    global _FLOORS
    sq, sq32 = {}, {}
    for smp in range(GRAD_FLOOR_SAMPLES):
        c, s = content, style
        if smp:
            c, s = ulp_perturbed(content, 7000 + 2 * smp), ulp_perturbed(style, 7001 + 2 * smp)
        g64 = oracle64(torch.from_numpy(c).double(), torch.from_numpy(s).double())
        g32 = oracle32(torch.from_numpy(c), torch.from_numpy(s)) if oracle32 else {}
        named = step(c, s)
        if smp == 0:
            grad_bar(family, i, next(iter(g64)))  # loads _FLOORS
            for name, ref in g64.items():
                if name in skip:  # (exact-zero gradients: a probe scaled by ~0)
                    continue
                pin = probe_err(grad_probe(name, ref), _FLOORS[f"{family}/{i}/p64:{name}"],
                                ref.numel())
                assert pin < 1e-9, (family, i, name, "oracle float64 off the reference's", pin)
        for name, ref in g64.items():
            if name not in skip:
                sq[name] = sq.get(name, 0.0) + rel_l2(named[name].grad, ref) ** 2
                if name in g32:
                    sq32[name] = sq32.get(name, 0.0) + rel_l2(g32[name], ref) ** 2
    worst = 0.0
    for name, v in sq.items():
        e = float(np.sqrt(v / GRAD_FLOOR_SAMPLES))
        f32 = float(np.sqrt(sq32[name] / GRAD_FLOOR_SAMPLES)) if name in sq32 else 0.0
        bar = max(grad_bar(family, i, name), 3.0 * f32)
        if os.environ.get("RPST_GRAD_DEBUG"):
            print(f"GRADDBG {family} {i} {name} rms {e:.3e} cpu_bar {grad_bar(family, i, name):.3e} "
                  f"gpu32 {f32:.3e}")
        worst = max(worst, e / bar * 1e-4)
        assert e < bar, (family, i, name, "rms", e, bar)
    return worst

"""SANet attention backward over query chunks (rpst_sanet_attention_backward_chunked, the
training path of sanet.py:82-99 under autograd): dF, dG, dH against
float64 torch autograd of O = H softmax(F^T G)^T, with a ragged last query chunk (HW = 2400
= 2048 + 352), two chunks at C = 512 (HW = 4096), HWc != HWs (1200 queries, 2100 keys) and
one chunk (HW = 600). Tolerance rel-L2 1e-5 (fp32 vs fp64, logits of moderate spread).
The workspace has no B x HW x HW term. The single pass (rpst_sanet_attention_backward, S and
dP whole) is the same walk with one chunk: checked against the chunked entry bit for bit.
Peaked rows (|S| to 117, the regime training runs in) over several tiles, on both entries:
test_sanet_attention_backward_peaked_rows, bars from the CPU float32 form's own error."""
import copy

import pytest
import torch

from helpers import flat_or_live, rel_l2
from train_glue_ref import (ATTN_GRADS, ATTN_PEAKED, attn_peaked_case, row_peak_median,
                            row_sum_residue)

pytestmark = pytest.mark.gpu


def _ref_grads(F, G, H, dO):
    F, G, H = (x.double().clone().requires_grad_(True) for x in (F, G, H))
    B, C, hw = F.shape
    P = torch.softmax(torch.bmm(F.transpose(1, 2), G), -1)
    O = torch.bmm(H, P.transpose(1, 2))
    (O * dO.double()).sum().backward()
    return O.detach(), F.grad, G.grad, H.grad


@pytest.mark.parametrize("shape", [(2, 64, 2400, 2400), (1, 512, 4096, 4096),
                                   (2, 48, 1200, 2100), (2, 64, 600, 600)])
def test_sanet_attention_backward_chunked(cuda, shape):
    from rpst import _lib, ops
    B, C, hw, hws = shape
    g = torch.Generator(device=cuda).manual_seed(3)
    F = torch.randn((B, C, hw), device=cuda, generator=g) * (2.0 / C ** 0.5)
    G = torch.randn((B, C, hws), device=cuda, generator=g)
    H = torch.randn((B, C, hws), device=cuda, generator=g)
    dO = torch.randn((B, C, hw), device=cuda, generator=g)
    O, dF_ref, dG_ref, dH_ref = _ref_grads(F, G, H, dO)
    lib = _lib.load()
    nbytes = lib.rpst_sanet_attention_backward_chunked_workspace_size(B, C, hw, hws)
    q = min(hw, 2048)  # S and dP of one 2048-query chunk + 2 row vectors: no B x HW x HW term
    assert nbytes == 4 * (2 * B * q * hws + 2 * B * q), nbytes
    ws = torch.empty(nbytes, device=cuda, dtype=torch.uint8)
    dF, dG, dH = (torch.empty_like(x) for x in (F, G, H))
    _lib.call("rpst_sanet_attention_backward_chunked", F.data_ptr(), G.data_ptr(), H.data_ptr(),
              dO.data_ptr(), dF.data_ptr(), dG.data_ptr(), dH.data_ptr(), B, C, hw, hws,
              ws.data_ptr(), nbytes, ops._stream(F))
    for got, ref, name in ((dF, dF_ref, "dF"), (dG, dG_ref, "dG"), (dH, dH_ref, "dH")):
        assert rel_l2(got, ref) < 1e-5, (name, rel_l2(got, ref))
    # the softmax is shift invariant per row: dS rows sum to ~0, so sum_j dG[c][j] = F dS 1 ~ 0
    # (fp64: ~1e-16; fp32 rounding of the 4096-term sums reads ~1e-5 of max|dG|)
    gsum = dG.double().sum(-1).abs().max() / dG.double().abs().max()
    assert gsum < 5e-5, float(gsum)


@pytest.mark.parametrize("shape", [(1, 16, 2100, 68), (2, 48, 72, 100)])
def test_sanet_attention_backward_single_pass(cuda, shape):
    """rpst_sanet_attention_backward (S and dP whole) against the chunked entry and float64
    autograd. (1, 16, 2100, 68) crosses the 2048-query seam (2048 + 52 queries) with a tiny S;
    (2, 48, 72, 100) is one chunk with C, HWc and HWs all ragged against the 128 x 128 x 32
    tile. dF is bit-equal between the two on both shapes: each dF column's sums run over the
    keys only, in the same order, and dS does not depend on the chunk. dG and dH sum over the
    queries, so they are bit-equal only where there is one chunk. Tolerance rel-L2 1e-5 as
    above (torch fp32 against float64 reads 2.7e-7 to 4.4e-7 on these gradients on a CPU)."""
    from rpst import _lib, ops
    B, C, hw, hws = shape
    g = torch.Generator(device=cuda).manual_seed(3)
    F = torch.randn((B, C, hw), device=cuda, generator=g) * (2.0 / C ** 0.5)
    G = torch.randn((B, C, hws), device=cuda, generator=g)
    H = torch.randn((B, C, hws), device=cuda, generator=g)
    dO = torch.randn((B, C, hw), device=cuda, generator=g)
    refs = _ref_grads(F, G, H, dO)[1:]
    lib = _lib.load()
    single = lib.rpst_sanet_attention_backward_workspace_size(B, hw, hws)
    assert single == 4 * (2 * B * hw * hws + 2 * B * hw), single
    chunked = lib.rpst_sanet_attention_backward_chunked_workspace_size(B, C, hw, hws)
    got = {}
    for fn, nbytes in (("rpst_sanet_attention_backward", single),
                       ("rpst_sanet_attention_backward_chunked", chunked)):
        ws = torch.empty(nbytes, device=cuda, dtype=torch.uint8)
        got[fn] = tuple(torch.empty_like(x) for x in (F, G, H))
        _lib.call(fn, F.data_ptr(), G.data_ptr(), H.data_ptr(), dO.data_ptr(),
                  *(x.data_ptr() for x in got[fn]), B, C, hw, hws, ws.data_ptr(), nbytes,
                  ops._stream(F))
        for x, ref, name in zip(got[fn], refs, ("dF", "dG", "dH")):
            print(fn, shape, name, rel_l2(x, ref))
            assert rel_l2(x, ref) < 1e-5, (fn, name, rel_l2(x, ref))
    one, many = got.values()
    assert torch.equal(one[0], many[0]), "dF"
    if hw <= 2048:
        assert torch.equal(one[1], many[1]), "dG"
        assert torch.equal(one[2], many[2]), "dH"


@pytest.mark.parametrize("case", ATTN_PEAKED)
def test_sanet_attention_backward_peaked_rows(cuda, case):
    """Both entries on peaked rows over several tiles, the regime training runs in (at
    relu4_1 the logits span ~100 per row): the tests above feed moderate logits (|S| <= 10,
    median largest probability 0.1), and the peaked rows of test_sanet_backward have at most 64
    keys, one lane pass of the row kernels, one GEMM tile and one query chunk. The cases
    (train_glue_ref.ATTN_PEAKED: uniform F, G scaled by 3, 2 or 1) reach |S| of 38 to 117
    with ragged tiles and HWc != HWs, a C off the 16-byte path, one element past a tile on both
    sides, the 2048-query seam, and C = 512 over 8 x 8 tiles. The reference is _ref_grads'
    float64 autograd, formed once on the CPU and shared with tests/test_train_glue_cpu.py
    (train_glue_ref.attn_peaked_case). On it the
    median over the rows of the largest probability is >= 0.7. dF, dG, dH are finite and
    each within max(1e-5, 3 x the CPU float32 torch form's rel-L2 against float64), a bar
    that never passes 1e-4 (the factor 3 is _floor_bars'). Between the entries: dF bit-equal,
    dG and dH bit-equal where HWc <= 2048. sum_j dG[c][j] ~ 0 at the chunked test's bar, 5e-5 of
    max|dG|, the CPU float32 form's own residue printed beside it."""
    from rpst import _lib, ops
    B, C, hw, hws, _ = case
    inputs, S, P, g64, f32 = attn_peaked_case(case)
    peak = row_peak_median(P)
    print(f"peaked rows {case}: |S| max {float(S.abs().max()):.1f}, peak median {peak:.3f}")
    assert peak >= 0.7, peak
    bars = {k: max(1e-5, 3.0 * f32[k]) for k in ATTN_GRADS}
    assert all(b <= 1e-4 for b in bars.values()), bars
    F, G, H, dO = (x.to(cuda) for x in inputs)
    lib = _lib.load()
    sizes = (("rpst_sanet_attention_backward",
              lib.rpst_sanet_attention_backward_workspace_size(B, hw, hws)),
             ("rpst_sanet_attention_backward_chunked",
              lib.rpst_sanet_attention_backward_chunked_workspace_size(B, C, hw, hws)))
    got = {}
    for fn, nbytes in sizes:
        ws = torch.empty(nbytes, device=cuda, dtype=torch.uint8)
        got[fn] = dict(zip(ATTN_GRADS, (torch.empty_like(x) for x in (F, G, H))))
        _lib.call(fn, F.data_ptr(), G.data_ptr(), H.data_ptr(), dO.data_ptr(),
                  *(got[fn][k].data_ptr() for k in ATTN_GRADS), B, C, hw, hws, ws.data_ptr(),
                  nbytes, ops._stream(F))
    errs = {fn: {k: rel_l2(g[k], g64[k]) for k in ATTN_GRADS} for fn, g in got.items()}
    gsums = {fn: row_sum_residue(g["dG"]) for fn, g in got.items()}
    for fn in got:
        for k in ATTN_GRADS:
            print(f"{fn} {case} {k}: rel-L2 {errs[fn][k]:.3e} (bar {bars[k]:.3e}, "
                  f"fp32 {f32[k]:.3e})")
        print(f"{fn} {case} dG row sums: {gsums[fn]:.3e} (bar 5e-05, fp32 {f32['gsum']:.3e})")
    for fn, g in got.items():
        for k in ATTN_GRADS:
            assert torch.isfinite(g[k]).all(), (fn, k)
            assert errs[fn][k] < bars[k], (fn, k, errs[fn][k], bars[k])
        assert gsums[fn] < 5e-5, (fn, gsums[fn])
    one, many = got.values()
    assert torch.equal(one["dF"], many["dF"]), "dF"
    if hw <= 2048:
        assert torch.equal(one["dG"], many["dG"]), "dG"
        assert torch.equal(one["dH"], many["dH"]), "dH"


@pytest.mark.parametrize("mode,inputs", flat_or_live([("aea", ("aea",)), ("relu", ("relu",))]))
def test_adaptive_attention_backward_query_chunks(cuda, mode, inputs):
    """rpst_adaptive_attention_backward over query chunks (HW = 2400: 2048 + 352): all seven
    gradients of O = H AEA(A, softmax(F^T G))^T against float64 torch autograd of the oracle's
    restatement (R.aea), and a workspace with no B x HW x HW term.
    flat: F and G are normal x 0.2, so P ~ 1 / HW (max 0.0027) and the clamp is dead. dF, dG, dH
    within 1e-5, the f_psi gradients within max(1e-5, 3 x the oracle's own fp32 distance to
    float64); with 'relu' no entry of P passes its clamp, so dF, dG and the f_psi gradients are
    exactly zero on both sides, and that is what is asserted of them.
    live: F and G from helpers.peaked_attention_inputs, all seven under the conditions and
    bars of helpers.aea_live_bars."""
    import network as net
    from helpers import (aea_attention_grads, aea_backward_abi, aea_fp32_forms, aea_live_bars,
                         check_aea_grads, clamp_liveness, peaked_attention_inputs, state_dict_of,
                         synth_)
    B, C, h, w = 1, 64, 40, 60
    hw = h * w
    mod = net.AEAModule(hw) if mode == "aea" else net.AEALReluModule(hw)
    synth_(mod, 13)
    g = torch.Generator(device=cuda).manual_seed(4)
    F = torch.randn((B, C, hw), device=cuda, generator=g) * 0.2
    G = torch.randn((B, C, hw), device=cuda, generator=g) * 0.2
    H = torch.randn((B, C, hw), device=cuda, generator=g)
    c = torch.rand((B, C, hw), device=cuda, generator=g)
    s = torch.rand((B, C, hw), device=cuda, generator=g)
    dO = torch.randn((B, C, hw), device=cuda, generator=g)
    if inputs == "live":
        F, G = (x.view(B, C, hw).to(cuda) for x in peaked_attention_inputs(B, C, h, w, 3))
    host = [x.cpu().view(B, C, h, w) for x in (F, G, H, c, s, dO)]
    sd = state_dict_of(mod)
    _, clamp, P, Q, g64 = aea_attention_grads(*host, sd, mode, torch.float64)
    g32s = aea_fp32_forms(*host, sd, mode)
    what = f"query chunks {mode} {inputs}"
    got, nbytes = aea_backward_abi(mod.to(cuda), F, G, H, c, s, dO)
    assert nbytes < 2 * B * hw * hw * 4, nbytes  # the single pass's S and dQ alone
    if inputs == "live":
        check_aea_grads(got, g64, aea_live_bars(g32s, g64, P, Q, clamp, mode), what)
        return
    assert clamp_liveness(P, clamp, mode) == 0.0
    dead = ("dF", "dG") + tuple(k for k in g64 if k.startswith("f_psi")) if mode == "relu" else ()
    for k in dead:  # relu never active: zero on both sides, exactly
        assert not g64[k].any() and not got[k].any(), k
    bars = {k: 1e-5 if k in ("dF", "dG", "dH")
            else max(1e-5, 3.0 * max(rel_l2(g32[k], g64[k]) for g32 in g32s))
            for k in g64 if k not in dead}
    check_aea_grads(got, {k: g64[k] for k in bars}, bars, what)


@pytest.mark.parametrize("mode", ("aea", "relu"))
@pytest.mark.parametrize("shape", [(2, 48, 8, 10), (3, 64, 9, 7), (1, 512, 32, 32),
                                   (1, 64, 35, 60)])
def test_adaptive_attention_backward_live_clamp(cuda, mode, shape):
    """rpst_adaptive_attention_backward where the AEA clamp is live: every query has one
    dominant key whose probability is spread over [0.3, 0.97] (helpers.peaked_attention_inputs),
    so the sigmoid's mid-range and both tails ('aea'), the ReLU mask and the second softmax
    ('relu'), dc = -sum dP and the chain into f_psi all carry weight. Shapes: C = 48 is no
    flash width (the forward's GEMM path forms S) with hid = 5; HW = 63 is odd (no 16-byte
    rows), hid = 3, three images; (1, 512, 32, 32) is the production width, hid = 64;
    HW = 2100 crosses the 2048-query chunk seam with a 52-row last chunk. The forward with
    keep_claims at the bars of test_adaptive_attention_peaked, then all seven gradients against
    float64 autograd of the oracle's restatement, each within max(1e-5, 3 x the oracle's own
    fp32 CPU autograd's distance to float64, in the worse of its two forms)
    (helpers.aea_live_case and aea_live_bars, which also assert the liveness conditions and
    that no bar passes 1e-4; the generator's seed is 3, and 10 at C = 512), and a second call
    bit for bit (the sums are fixed-order)."""
    from rpst import ops
    from helpers import aea_backward_abi, aea_live_case, check_aea_grads
    case = aea_live_case(mode, shape)
    mod = copy.deepcopy(case.mod).to(cuda)
    F, G, H, c, s, dO = (x.to(cuda) for x in (case.F, case.G, case.H, case.c, case.s, case.dO))
    with torch.no_grad():
        out, cl, before, after = ops.adaptive_attention(F, G, H, c, s, mod.f_psi, mod.mode, 50.0,
                                                        0.4, 0.5, keep_claims=True)
    for got, ref, bar, name in ((cl, case.clamp, 1e-6, "clamp"), (before, case.P, 1e-5, "before"),
                                (after, case.Q, 1e-5, "after"), (out, case.out, 1e-5, "out")):
        print(f"live clamp {mode} {shape} {name}: rel-L2 {rel_l2(got, ref):.3e} (bar {bar:.0e})")
        assert rel_l2(got, ref) < bar, (name, rel_l2(got, ref))
    got, _ = aea_backward_abi(mod, F, G, H, c, s, dO)
    check_aea_grads(got, case.g64, case.bars, f"live clamp {mode} {shape}")
    again, _ = aea_backward_abi(mod, F, G, H, c, s, dO)
    for k in got:
        assert torch.equal(got[k], again[k]), k

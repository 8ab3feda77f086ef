"""C-ABI checks that need no GPU: the library loads, exports every symbol the header
declares (the ctypes table is derived from the header: tests/test_abi_header.py), a stale
library is refused by name, and argument validation reports errors through status codes +
rpst_last_error() without touching the device."""
import ctypes
import os
import re

import pytest

from rpst import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rpst.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rpst_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_functions():
    fns = header_functions()
    assert "rpst_conv2d" in fns and "rpst_adain" in fns and len(fns) >= 10


def test_library_exports_every_header_symbol():
    lib = _lib.load()
    for name in header_functions():
        assert hasattr(lib, name), f"{name} declared in rpst.h but not exported"


def test_stale_library_is_named():
    """A library that lacks a symbol the header declares (an old build) is refused with the
    symbol's name and the advice to rebuild, not with a bare AttributeError."""
    table = dict(_lib.SIGNATURES, rpst_added_since_the_build=(ctypes.c_int, [ctypes.c_int]))
    with pytest.raises(_lib.RpstError, match="rpst_added_since_the_build.*rebuild"):
        _lib._bind(ctypes.CDLL(_lib.LIB_PATH), table)
    assert "rpst_added_since_the_build" not in _lib.SIGNATURES
    _lib._bind(ctypes.CDLL(_lib.LIB_PATH), dict(_lib.SIGNATURES))


def test_version_and_error_string():
    lib = _lib.load()
    assert lib.rpst_version() >= 100
    assert isinstance(lib.rpst_last_error(), bytes)


def test_size_queries_are_host_only():
    lib = _lib.load()
    assert lib.rpst_adain_workspace_size(2, 3) == 4 * 4 * 6
    # 3x3, Cin=3 -> one chunk of 8 channels, Cout=16 padded to 32 (direct image), then
    # the F(2x2) Winograd image: Cout padded to 32, 16 transformed taps per (co, ci), then
    # the F(4x4) image: one (32-channel co tile, 8-channel chunk) slice of 36 taps, then the
    # position-quarter F(4x4) image: one (64-channel co tile, 4-channel K step) slice
    assert lib.rpst_conv2d_packed_size(16, 3, 3) == (1 * 9 * 8 * 32 + 32 * 8 * 16 + 36 * 32 * 8 +
                                                     36 * 64 * 4) * 4
    assert lib.rpst_conv2d_packed_size(16, 3, 1) == 1 * 16 * 32 * 4
    assert lib.rpst_conv2d_packed_size(16, 3, 2) == 0


WCT_SIZES = {(3, 16, 35): 1075840, (1, 64, 1023): 1796720, (1, 64, 8192): 1796720,
             (2, 128, 384): 8268896, (2, 256, 256): 33054816, (1, 200, 117): 10090128,
             (1, 160, 351): 6458832, (1, 320, 256): 25820880, (1, 272, 117): 18658128,
             (1, 320, 8192): 27459280, (16, 256, 262144): 1321402688,
             (16, 512, 4096): 503677152, (1, 512, 2): 66089040}
POWER_SIZES = {(96, 3): 2876208, (64, 1): 426080, (256, 16): 109068440, (512, 2): 54534184,
               (1000, 1): 104016416}
RETIRED_WCT_KNOBS = {"RPST_WCT_KMIN": "1024", "RPST_WCT_COV_BT": "64", "RPST_WCT_COV_V2": "0",
                     "RPST_WCT_T_BT": "128", "RPST_COV_COMPACT": "0"}


def test_wct_workspace_sizes_are_pinned(monkeypatch):
    """rpst_wct_workspace_size(n, C, HW) and rpst_matrix_power_workspace_size(n, batch) are
    host-only functions of their arguments: the retired RPST_WCT_* / RPST_COV_* switches no
    longer move them (a workspace sized under one environment serves a call under another)."""
    lib = _lib.load()

    def check():
        for args, nbytes in WCT_SIZES.items():
            assert lib.rpst_wct_workspace_size(*args) == nbytes, args
        for args, nbytes in POWER_SIZES.items():
            assert lib.rpst_matrix_power_workspace_size(*args) == nbytes, args

    for k in RETIRED_WCT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    check()
    for k, v in RETIRED_WCT_KNOBS.items():
        monkeypatch.setenv(k, v)
        check()
        monkeypatch.delenv(k)


def _wct_entry_args(entry, first=1, n=2, C=16, HW=64, short=0):
    """Arguments of a WCT entry point with placeholder pointers (every case below fails its
    argument checks, which run before any launch). n / C / HW: batch, channels, pixels; for
    rpst_matrix_power_psd_f64 the batch and the matrix size. short: bytes the workspace lacks."""
    lib = _lib.load()
    n1 = 1 if "whiten" in entry else n
    ws = max(lib.rpst_wct_workspace_size(n1, C, HW) - short, 0)
    pw = max(lib.rpst_matrix_power_workspace_size(C, n) - short, 0)
    return {
        "rpst_wct_fuse": (first, 1, 1, n, C, HW, None, 1, ws, None),
        "rpst_wct_params": (first, 1, None, 1, 1, n, C, HW, None, 1, ws, None),
        "rpst_whiten_and_color_f64": (first, 1, 1, C, HW, None, 1, ws, None),
        "rpst_whiten_and_color_original_f64": (first, 1, 1, C, HW, 1, ws, None),
        "rpst_wct_status": (first, n, C, HW, 1, None),
        "rpst_whiten_and_color_status": (first, C, HW, 1, None),
        "rpst_matrix_power_psd_f64": (first, 1, C, n, 0, None, 1, pw, None),
    }[entry]


# (entry, defect) -> (status, rpst_last_error()), as the entries answered before they shared
# one check: RPST_EINVAL -1, RPST_EWORKSPACE -3
WCT_ERRORS = {
    ("rpst_wct_fuse", "null"): (-1, "wct_fuse: null pointer"),
    ("rpst_wct_fuse", "n=0"): (-1, "wct_fuse: bad shape n=0 C=16 HW=64"),
    ("rpst_wct_fuse", "HW=1"): (-1, "wct_fuse: bad shape n=2 C=16 HW=1"),
    ("rpst_wct_fuse", "C=1025"): (-1, "wct_fuse: shape too large"),
    ("rpst_wct_fuse", "short"): (-3, "wct_fuse: workspace 717239 < 717240 bytes"),
    ("rpst_wct_params", "null"): (-1, "wct_params: null pointer"),
    ("rpst_wct_params", "n=0"): (-1, "wct_params: bad shape n=0 C=16 HW=64"),
    ("rpst_wct_params", "HW=1"): (-1, "wct_params: bad shape n=2 C=16 HW=1"),
    ("rpst_wct_params", "C=1025"): (-1, "wct_params: C=1025 > 1024"),
    ("rpst_wct_params", "short"): (-3, "wct_params: workspace 717239 < 717240 bytes"),
    ("rpst_whiten_and_color_f64", "null"): (-1, "whiten_and_color: null pointer"),
    ("rpst_whiten_and_color_f64", "HW=1"): (-1, "whiten_and_color: bad shape"),
    ("rpst_whiten_and_color_f64", "C=1025"): (-1, "whiten_and_color: bad shape"),
    ("rpst_whiten_and_color_f64", "short"): (-3, "whiten_and_color: workspace too small"),
    ("rpst_whiten_and_color_original_f64", "null"):
        (-1, "whiten_and_color(original): null pointer"),
    ("rpst_whiten_and_color_original_f64", "HW=1"): (-1, "whiten_and_color(original): bad shape"),
    ("rpst_whiten_and_color_original_f64", "C=1025"):
        (-1, "whiten_and_color(original): bad shape"),
    ("rpst_whiten_and_color_original_f64", "short"):
        (-3, "whiten_and_color(original): workspace too small"),
    ("rpst_wct_status", "null"): (-1, "wct_status: null pointer"),
    ("rpst_wct_status", "n=0"): (-1, "wct_status: bad shape"),
    ("rpst_wct_status", "HW=1"): (-1, "wct_status: bad shape"),
    ("rpst_wct_status", "C=1025"): (-1, "wct_status: bad shape"),
    ("rpst_whiten_and_color_status", "null"): (-1, "whiten_and_color_status: null pointer"),
    ("rpst_whiten_and_color_status", "HW=1"): (-1, "whiten_and_color_status: bad shape"),
    ("rpst_whiten_and_color_status", "C=1025"): (-1, "whiten_and_color_status: bad shape"),
    ("rpst_matrix_power_psd_f64", "null"): (-1, "matrix_power: null pointer"),
    ("rpst_matrix_power_psd_f64", "n=0"): (-1, "matrix_power: bad shape"),
    ("rpst_matrix_power_psd_f64", "C=1025"): (-1, "matrix_power: bad shape"),
    ("rpst_matrix_power_psd_f64", "short"): (-3, "matrix_power: workspace too small"),
}
WCT_DEFECTS = {"null": {"first": None}, "n=0": {"n": 0}, "HW=1": {"HW": 1}, "C=1025": {"C": 1025},
               "short": {"short": 1}}


@pytest.mark.parametrize("entry,defect", list(WCT_ERRORS))
def test_wct_entry_argument_errors(entry, defect):
    """Every WCT entry point answers a null pointer, a bad shape (n = 0, HW = 1, C = 1025: for
    rpst_matrix_power_psd_f64 a zero batch and a 1025 x 1025 matrix) and a workspace one byte
    short with its own status code and message, before any launch (no GPU needed)."""
    lib = _lib.load()
    status, message = WCT_ERRORS[(entry, defect)]
    assert getattr(lib, entry)(*_wct_entry_args(entry, **WCT_DEFECTS[defect])) == status
    error = lib.rpst_last_error().decode()
    assert error == message
    assert error.startswith(entry[len("rpst_"):].replace("_f64", "").replace(
        "_original", "(original)").replace("_psd", "") + ":")


@pytest.mark.parametrize("args,msg", [
    ((None, None, None, None, None, None, 1, 3, 8, 8, 16, 3, 0, 0, 1, None), "null pointer"),
    ((1, None, 1, None, None, 1, 1, 3, 8, 8, 16, 5, 0, 0, 1, None), "ksize"),
    ((1, None, 1, None, None, 1, 1, 3, 8, 8, 16, 3, 7, 0, 1, None), "bad pad"),
    ((1, None, 1, None, None, 1, 1, 3, 1, 8, 16, 3, 1, 0, 1, None), "reflect padding"),
    ((1, None, 1, None, None, 1, 1, 3, 8, 8, 16, 3, 0, 3, 1, None), "aux"),
])
def test_conv2d_argument_errors(args, msg):
    lib = _lib.load()
    st = lib.rpst_conv2d(*args)
    assert st == -1
    assert msg in lib.rpst_last_error().decode()
    with pytest.raises(_lib.RpstError, match=msg):
        _lib.call("rpst_conv2d", *args)


def test_conv2d_mix_refuses_ksize_before_the_layout():
    """rpst_conv2d_mix refuses a ksize other than 1 or 3 with conv2d's status and wording
    before it lays out its workspace: that ksize sizes as 0 bytes, which any workspace
    satisfies, and the layer's fallback writes z = T x + c into the workspace ahead of the
    conv's own ksize check. Placeholder pointers: the refusal comes before any launch."""
    lib = _lib.load()
    assert lib.rpst_conv2d_mix_workspace_size(2, 8, 9, 13, 32, 5) == 0
    args = (1, 1, 1, 1, None, 1, 2, 8, 9, 13, 32, 5, 0, 0, None, 0, None)
    assert lib.rpst_conv2d_mix(*args) == -1
    assert lib.rpst_last_error().decode() == "conv2d_mix: ksize must be 1 or 3, got 5"
    with pytest.raises(_lib.RpstError, match="ksize must be 1 or 3, got 5"):
        _lib.call("rpst_conv2d_mix", *args)
    assert lib.rpst_conv2d_mix_workspace_size(2, 8, 9, 13, 32, 5) == 0


@pytest.mark.parametrize("n1,n,msg", [(0, 4, "0 < n1 <= N"), (5, 4, "0 < n1 <= N"),
                                       (2, 4, "null second input")])
def test_conv2d_pair_argument_errors(n1, n, msg):
    """rpst_conv2d_pair checks its split before touching the device (no GPU needed)."""
    lib = _lib.load()
    x2 = None if msg == "null second input" else 1
    st = lib.rpst_conv2d_pair(1, x2, n1, 1, None, 1, n, 3, 8, 8, 16, 3, 0, 1, None)
    assert st == -1
    assert msg in lib.rpst_last_error().decode()


def test_conv2d_masked_argument_errors():
    """rpst_conv2d_masked needs its mask, and the mask epilogue carries no statistics."""
    lib = _lib.load()
    st = lib.rpst_conv2d_masked(1, 1, None, None, 1, 2, 16, 8, 8, 16, 3, 0, None)
    assert st == -1
    assert "null mask" in lib.rpst_last_error().decode()


def test_conv2d_pool_needs_the_f4x4_path():
    """rpst_conv2d_pool refuses a layer the library would not run on F(4x4) (a 3-channel
    input conv), before any launch."""
    lib = _lib.load()
    st = lib.rpst_conv2d_pool(1, None, 1, None, 1, 1, 3, 16, 16, 16, 3, 0, 0, 1, None)
    assert st == -1
    assert "F(4x4)" in lib.rpst_last_error().decode()


def test_adain_workspace_error():
    lib = _lib.load()
    st = lib.rpst_adain(1, 1, 1, 2, 3, 16, ctypes.c_float(1e-5), 1, 8, None)
    assert st == -3
    assert "workspace" in lib.rpst_last_error().decode()


def test_cpu_tensors_raise_no_fallback():
    import torch
    import network as net
    x = torch.rand(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        net.calc_mean_std(x)
    m = net.AdaINRPNet({"rp_blocks": 3, "hidden_dim": 2}, net.vgg)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.test(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))


def test_conv_algorithm_choice_is_host_only(monkeypatch):
    """rpst_conv2d_algorithm: the VALU narrow kernel for the 3->16 / 16->3 shapes, direct
    for the other layers below 16 input channels, else F(4x4) for the NONE / ADAIN /
    UPSAMPLE2 loaders, F(2x2) for the other 3x3 layers with Cout >= 32, direct otherwise;
    precise mode (training), RPST_CONV_ALGO and RPST_CONV_NARROW override."""
    monkeypatch.delenv("RPST_CONV_ALGO", raising=False)
    monkeypatch.delenv("RPST_CONV_NARROW", raising=False)
    lib = _lib.load()
    D, W2, W4, NR = 0, 1, 2, 3
    assert lib.rpst_conv2d_algorithm(256, 128, 512, 512, 3, 0) == W4
    assert lib.rpst_conv2d_algorithm(128, 256, 512, 512, 3, 4) == W4   # AdaIN-in-loader
    assert lib.rpst_conv2d_algorithm(256, 256, 32, 32, 3, 2) == W4     # upsample
    assert lib.rpst_conv2d_algorithm(128, 64, 64, 64, 3, 1) == W2      # max-pool loader
    assert lib.rpst_conv2d_algorithm(64, 3, 512, 512, 3, 0) == W4       # 3-channel input
    assert lib.rpst_conv2d_algorithm(64, 8, 512, 512, 3, 0) == D        # 8-channel input
    assert lib.rpst_conv2d_algorithm(3, 32, 512, 512, 3, 5) == NR       # skip-AdaIN 32->3
    assert lib.rpst_conv2d_algorithm(3, 64, 512, 512, 3, 0) == NR       # VGG decoder 64->3
    assert lib.rpst_conv2d_algorithm(3, 128, 512, 512, 3, 0) != NR      # Cin > 64
    assert lib.rpst_conv2d_algorithm(16, 3, 512, 512, 3, 0) == NR      # RP 3->16
    assert lib.rpst_conv2d_algorithm(3, 16, 512, 512, 3, 0) == NR      # RP 16->3
    assert lib.rpst_conv2d_algorithm(8, 8, 512, 512, 3, 0) == D        # not narrow_shape
    assert lib.rpst_conv2d_algorithm(3, 16, 512, 512, 3, 1) == D       # loader op: MFMA path
    # narrow grid threads: 64 columns x 16 rows (Cout <= 4: 4 rows per thread) per block
    assert lib.rpst_conv2d_grid_threads(2, 16, 512, 512, 3, 3, 0) == 2 * 8 * 32 * 256
    assert lib.rpst_conv2d_grid_threads(2, 3, 512, 512, 16, 3, 0) == 2 * 8 * 64 * 256
    monkeypatch.setenv("RPST_CONV_NARROW", "0")
    assert lib.rpst_conv2d_algorithm(3, 16, 512, 512, 3, 0) == W4
    assert lib.rpst_conv2d_algorithm(16, 3, 512, 512, 3, 0) == W4     # 3-channel input: F(4x4)
    monkeypatch.delenv("RPST_CONV_NARROW")
    assert lib.rpst_conv2d_algorithm(16, 32, 512, 512, 3, 0) == W4
    assert lib.rpst_conv2d_algorithm(512, 512, 64, 64, 1, 0) == D
    old = lib.rpst_conv2d_set_precise(1)
    try:
        assert lib.rpst_conv2d_algorithm(256, 128, 512, 512, 3, 0) == W2
    finally:
        lib.rpst_conv2d_set_precise(old)
    old = lib.rpst_conv2d_set_precise(2)   # training constant branch: F(4x4), 32-channel form
    try:
        assert lib.rpst_conv2d_algorithm(256, 128, 512, 512, 3, 0) == W4
        assert lib.rpst_conv2d_set_precise(2) == 2
    finally:
        lib.rpst_conv2d_set_precise(old)
    assert lib.rpst_conv2d_algorithm(256, 128, 512, 512, 3, 0) == W4
    monkeypatch.setenv("RPST_CONV_ALGO", "direct")
    assert lib.rpst_conv2d_algorithm(256, 128, 512, 512, 3, 0) == D
    assert lib.rpst_conv2d_algorithm(3, 16, 512, 512, 3, 0) == NR


def test_quarter_kernel_switch_is_per_launch(monkeypatch):
    """rpst_conv2d_quarter / rpst_conv2d_set_quarter: the position-quarter F(4x4) kernel takes
    the Cin >= 128 layers by default; RPST_W4Q is read per launch (0 off, 2 forced on every
    shape it supports) and the thread-local setter overrides it; precise level 2 keeps the
    32-channel form. Workspace sizes do not depend on the setting; the stats and fold sizes do
    not depend on the precise level either (the mix size does: at level 1 it holds T x + c)."""
    monkeypatch.delenv("RPST_CONV_ALGO", raising=False)
    monkeypatch.delenv("RPST_W4Q", raising=False)
    lib = _lib.load()
    q = lib.rpst_conv2d_quarter
    assert q(256, 128, 512, 512, 3, 0) == 1
    assert q(128, 64, 512, 512, 3, 0) == 0           # Cin < 128: 32-channel kernel
    assert q(32, 128, 512, 512, 3, 0) == 0           # Cout < 64
    assert q(128, 128, 64, 64, 3, 1) == 0            # max-pool loader: F(2x2)
    assert q(64, 128, 23, 70, 3, 2) == 1             # upsample loader
    assert q(200, 144, 19, 90, 3, 0) == 1            # Cin % 16 == 0, partial co tile
    assert q(256, 136, 64, 64, 3, 0) == 0            # Cin % 16 != 0
    def sample():
        return (lib.rpst_conv2d_stats_workspace_size(2, 128, 37, 200, 256, 3, 0),
                lib.rpst_conv2d_workspace_size(2, 256, 37, 70, 96, 3, 4),
                lib.rpst_conv2d_mix_workspace_size(2, 128, 37, 70, 96, 3))

    def sample_levels():
        out = []
        for level in (0, 1, 2):
            p = lib.rpst_conv2d_set_precise(level)
            try:
                out.append(sample())
            finally:
                lib.rpst_conv2d_set_precise(p)
        return out

    sizes = sample()
    levels = sample_levels()
    assert levels[0] == sizes
    assert levels[0][:2] == levels[1][:2] == levels[2][:2] and levels[0][1] > 0
    monkeypatch.setenv("RPST_W4Q", "0")
    assert q(256, 128, 512, 512, 3, 0) == 0
    monkeypatch.setenv("RPST_W4Q", "2")
    assert q(128, 64, 512, 512, 3, 0) == 1
    assert q(64, 16, 512, 512, 3, 0) == 1
    assert q(32, 64, 512, 512, 3, 0) == 0            # Cout < 64 even when forced
    assert sample() == sizes
    assert sample_levels() == levels                 # per level, equal across quarter settings
    old = lib.rpst_conv2d_set_quarter(0)
    try:
        assert old == -1
        assert q(128, 64, 512, 512, 3, 0) == 0       # the setter wins over RPST_W4Q
        lib.rpst_conv2d_set_quarter(2)
        assert q(128, 64, 512, 512, 3, 0) == 1
        p = lib.rpst_conv2d_set_precise(2)
        try:
            assert q(256, 128, 512, 512, 3, 0) == 0  # training constant branch
        finally:
            lib.rpst_conv2d_set_precise(p)
    finally:
        lib.rpst_conv2d_set_quarter(old)
    monkeypatch.delenv("RPST_W4Q")
    assert q(128, 64, 512, 512, 3, 0) == 0


def test_grid_threads_reports_the_launched_grid(monkeypatch):
    """rpst_conv2d_grid_threads reads the plan the launch reads, the F(4x4) co-split included:
    128 -> 128 at 64x64 has 16 chunks of 8 channels (>= 32 K steps of 4) and 4 co tiles of 32,
    so the 32-channel form splits them over 2 blocks per spatial tile."""
    for k in ("RPST_CONV_ALGO", "RPST_W4Q", "RPST_CONV_NARROW"):
        monkeypatch.delenv(k, raising=False)
    lib = _lib.load()
    shape = (1, 128, 64, 64, 128, 3, 0)
    old = lib.rpst_conv2d_set_quarter(0)
    try:
        # one 64-column tile x four 16-row tiles x co-split 2, 512 threads
        assert lib.rpst_conv2d_grid_threads(*shape) == 1 * 4 * 2 * 512
    finally:
        lib.rpst_conv2d_set_quarter(old)
    assert lib.rpst_conv2d_quarter(128, 128, 64, 64, 3, 0) == 1
    # the quarter form: one column tile x eight 8-row tiles, 512 threads, no co-split
    assert lib.rpst_conv2d_grid_threads(*shape) == 1 * 8 * 512
    old = lib.rpst_conv2d_set_quarter(0)
    try:
        # three co tiles (Cout = 96) do not split
        assert lib.rpst_conv2d_grid_threads(1, 128, 64, 64, 96, 3, 0) == 4 * 512
    finally:
        lib.rpst_conv2d_set_quarter(old)


def test_plan_rejects_unfused_first_transform():
    """A plan whose first step is not a conv cannot fuse the WCT colour transform (first_mix)
    or an AdaIN input operator: run() must refuse instead of silently decoding raw features."""
    import torch
    from rpst import ops, plan

    steps = [plan.OpStep(ops.IN_UPSAMPLE2)]
    x = torch.zeros(1, 4, 2, 2)
    with pytest.raises(NotImplementedError, match="first_mix"):
        plan.run(steps, x, first_mix=(None, None))
    with pytest.raises(NotImplementedError, match="first_in_op"):
        plan.run(steps, x, first_in_op=ops.IN_ADAIN)
    with pytest.raises(NotImplementedError, match="first_mix"):
        plan.run([], x, first_mix=(None, None))


# ---- workspaces: every size export and every refusal, pinned ------------------------------
SIZE_ENV = ("RPST_CONV_ALGO", "RPST_CONV_NARROW", "RPST_W4Q", "RPST_WGRAD_TC", "RPST_SANET_FLASH")
# export (without rpst_ / _workspace_size) -> argument tuples, chosen to reach every branch of
# its layout: flash-eligible C (64 / 128 / 256 / 512 with HW % 4 == 0) and not, HW below and
# above the 2048-query chunk, B * HW off the 128-row column chunks, T larger than the logits;
# wgrad with both channel counts <= 32, one side <= 8 and wide, W off the segment width;
# conv1x1_wgrad's pixel split clamped at 16 and down at 1
WS_SHAPES = {
    "adain": [(2, 3), (1, 64), (0, 5)],
    "masked_adain": [(2, 3), (1, 64), (2, 512)],
    "resized_mean_std": [(5, 7), (0, 3)],
    "sanet_attention": [(2, 48), (1, 2304)],
    "sanet_attention_workspace_size_c": [(2, 24, 48), (2, 64, 64), (1, 64, 50), (1, 128, 2304),
                                         (1, 256, 64), (1, 512, 64)],
    "cosine_affinity": [(2, 24, 48), (1, 64, 2304)],
    "aea_clamp": [(2, 48, 16), (1, 2304, 8)],
    "adaptive_attention": [(2, 24, 48, 16), (2, 64, 64, 16), (1, 24, 2304, 16), (1, 512, 16, 64),
                           (1, 24, 16, 64), (3, 64, 43, 16)],
    "sanet_attention_backward": [(2, 48, 40), (1, 2304, 100)],
    "sanet_attention_backward_chunked": [(2, 64, 48, 40), (1, 64, 2304, 40), (1, 64, 2048, 8)],
    "adaptive_attention_backward": [(2, 64, 48, 16), (1, 24, 2304, 8), (2, 64, 64, 16),
                                    (3, 512, 16, 64)],
    "conv1x1_wgrad": [(1, 8, 8), (64, 512, 512), (8, 512, 512), (2, 100, 300)],
    "reflect_pad_border_grad": [(2, 3, 5, 7), (1, 64, 32, 48)],
    "conv_wgrad": [(2, 16, 9, 13, 32), (2, 64, 9, 13, 3), (2, 8, 9, 13, 64), (2, 64, 33, 70, 128),
                   (1, 128, 64, 256, 128), (4, 32, 64, 200, 32)],
    "conv7_wgrad": [(2, 3, 9, 13, 16), (1, 16, 40, 300, 3), (4, 64, 64, 64, 64)],
    "sq_diff": [()],
}
# the conv sizes, taken at every rpst_conv2d_set_precise level x rpst_conv2d_set_quarter setting
CONV_WS_SHAPES = {
    "conv2d_stats": [(2, 128, 37, 200, 256, 3, 0), (2, 3, 16, 16, 16, 3, 0),
                     (2, 64, 16, 16, 128, 1, 0), (2, 256, 37, 70, 96, 3, 4)],
    "conv2d": [(2, 256, 37, 70, 96, 3, 4), (2, 256, 37, 70, 96, 3, 0), (2, 8, 9, 13, 32, 3, 4)],
    "conv2d_mix": [(2, 128, 37, 70, 96, 3), (2, 8, 9, 13, 32, 3), (1, 16, 12, 20, 32, 3),
                   (2, 8, 9, 13, 32, 1), (2, 8, 9, 13, 32, 5)],
    "conv2d_gated": [(2, 32, 16, 16, 32, 1), (2, 32, 16, 16, 128, 1), (2, 32, 16, 16, 32, 3)],
}
CONV_MODES = [(level, quarter) for level in (0, 1, 2) for quarter in (-1, 0, 2)]


def _size_export(lib, name):
    return getattr(lib, f"rpst_{name}" if name.endswith("_c") else f"rpst_{name}_workspace_size")


def _workspace_sizes(lib):
    """{(export, arguments): bytes}; for the conv exports a tuple of bytes, one per CONV_MODES."""
    out = {(name, args): _size_export(lib, name)(*args)
           for name, shapes in WS_SHAPES.items() for args in shapes}
    conv = {(name, args): [] for name, shapes in CONV_WS_SHAPES.items() for args in shapes}
    for level, quarter in CONV_MODES:
        p, q = lib.rpst_conv2d_set_precise(level), lib.rpst_conv2d_set_quarter(quarter)
        try:
            for name, args in conv:
                conv[(name, args)].append(_size_export(lib, name)(*args))
        finally:
            lib.rpst_conv2d_set_precise(p)
            lib.rpst_conv2d_set_quarter(q)
    out.update({k: tuple(v) for k, v in conv.items()})
    return out


WS_SIZES = {('adain', (2, 3)): 96,
 ('adain', (1, 64)): 1024,
 ('adain', (0, 5)): 0,
 ('masked_adain', (2, 3)): 786432,
 ('masked_adain', (1, 64)): 4194304,
 ('masked_adain', (2, 512)): 8388608,
 ('resized_mean_std', (5, 7)): 48,
 ('resized_mean_std', (0, 3)): 0,
 ('sanet_attention', (2, 48)): 19200,
 ('sanet_attention', (1, 2304)): 21252096,
 ('sanet_attention_workspace_size_c', (2, 24, 48)): 19200,
 ('sanet_attention_workspace_size_c', (2, 64, 64)): 0,
 ('sanet_attention_workspace_size_c', (1, 64, 50)): 10400,
 ('sanet_attention_workspace_size_c', (1, 128, 2304)): 0,
 ('sanet_attention_workspace_size_c', (1, 256, 64)): 0,
 ('sanet_attention_workspace_size_c', (1, 512, 64)): 0,
 ('cosine_affinity', (2, 24, 48)): 18432,
 ('cosine_affinity', (1, 64, 2304)): 1179648,
 ('aea_clamp', (2, 48, 16)): 6912,
 ('aea_clamp', (1, 2304, 8)): 92160,
 ('adaptive_attention', (2, 24, 48, 16)): 45696,
 ('adaptive_attention', (2, 64, 64, 16)): 85504,
 ('adaptive_attention', (1, 24, 2304, 16)): 21888000,
 ('adaptive_attention', (1, 512, 16, 64)): 201152,
 ('adaptive_attention', (1, 24, 16, 64)): 13760,
 ('adaptive_attention', (3, 64, 43, 16)): 100104,
 ('sanet_attention_backward', (2, 48, 40)): 31488,
 ('sanet_attention_backward', (1, 2304, 100)): 1861632,
 ('sanet_attention_backward_chunked', (2, 64, 48, 40)): 31488,
 ('sanet_attention_backward_chunked', (1, 64, 2304, 40)): 671744,
 ('sanet_attention_backward_chunked', (1, 64, 2048, 8)): 147456,
 ('adaptive_attention_backward', (2, 64, 48, 16)): 116300,
 ('adaptive_attention_backward', (1, 24, 2304, 8)): 38494872,
 ('adaptive_attention_backward', (2, 64, 64, 16)): 168652,
 ('adaptive_attention_backward', (3, 512, 16, 64)): 635340,
 ('conv1x1_wgrad', (1, 8, 8)): 4096,
 ('conv1x1_wgrad', (64, 512, 512)): 67108864,
 ('conv1x1_wgrad', (8, 512, 512)): 67108864,
 ('conv1x1_wgrad', (2, 100, 300)): 3840000,
 ('reflect_pad_border_grad', (2, 3, 5, 7)): 2688,
 ('reflect_pad_border_grad', (1, 64, 32, 48)): 167936,
 ('conv_wgrad', (2, 16, 9, 13, 32)): 295424,
 ('conv_wgrad', (2, 64, 9, 13, 3)): 110640,
 ('conv_wgrad', (2, 8, 9, 13, 64)): 295936,
 ('conv_wgrad', (2, 64, 33, 70, 128)): 9748992,
 ('conv_wgrad', (1, 128, 64, 256, 128)): 37781504,
 ('conv_wgrad', (4, 32, 64, 200, 32)): 18890752,
 ('conv7_wgrad', (2, 3, 9, 13, 16)): 37888,
 ('conv7_wgrad', (1, 16, 40, 300, 3)): 471000,
 ('conv7_wgrad', (4, 64, 64, 64, 64)): 51396608,
 ('sq_diff', ()): 8192,
 ('conv2d_stats', (2, 128, 37, 200, 256, 3, 0)): (196608, 196608, 196608, 196608, 196608, 196608,
                                                  196608, 196608, 196608),
 ('conv2d_stats', (2, 3, 16, 16, 16, 3, 0)): (2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048,
                                              2048),
 ('conv2d_stats', (2, 64, 16, 16, 128, 1, 0)): (16384, 16384, 16384, 16384, 16384, 16384, 16384,
                                                16384, 16384),
 ('conv2d_stats', (2, 256, 37, 70, 96, 3, 4)): (11250440, 11250440, 11250440, 11250440, 11250440,
                                                11250440, 11250440, 11250440, 11250440),
 ('conv2d', (2, 256, 37, 70, 96, 3, 4)): (11213576, 11213576, 11213576, 11213576, 11213576,
                                          11213576, 11213576, 11213576, 11213576),
 ('conv2d', (2, 256, 37, 70, 96, 3, 0)): (0, 0, 0, 0, 0, 0, 0, 0, 0),
 ('conv2d', (2, 8, 9, 13, 32, 3, 4)): (0, 0, 0, 0, 0, 0, 0, 0, 0),
 ('conv2d_mix', (2, 128, 37, 70, 96, 3)): (7822360, 7822360, 7822360, 2785792, 2785792, 2785792,
                                           7822360, 7822360, 7822360),
 ('conv2d_mix', (2, 8, 9, 13, 32, 3)): (8640, 8640, 8640, 8640, 8640, 8640, 8640, 8640, 8640),
 ('conv2d_mix', (1, 16, 12, 20, 32, 3)): (241048, 241048, 241048, 17024, 17024, 17024, 241048,
                                          241048, 241048),
 ('conv2d_mix', (2, 8, 9, 13, 32, 1)): (8640, 8640, 8640, 8640, 8640, 8640, 8640, 8640, 8640),
 ('conv2d_mix', (2, 8, 9, 13, 32, 5)): (0, 0, 0, 0, 0, 0, 0, 0, 0),
 ('conv2d_gated', (2, 32, 16, 16, 32, 1)): (2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048),
 ('conv2d_gated', (2, 32, 16, 16, 128, 1)): (0, 0, 0, 0, 0, 0, 0, 0, 0),
 ('conv2d_gated', (2, 32, 16, 16, 32, 3)): (0, 0, 0, 0, 0, 0, 0, 0, 0)}


def test_workspace_sizes_are_pinned(monkeypatch):
    """Every *_workspace_size export returns exactly these bytes (host-only; the WCT sizes are
    pinned above)."""
    for k in SIZE_ENV:
        monkeypatch.delenv(k, raising=False)
    got = _workspace_sizes(_lib.load())
    assert list(got) == list(WS_SIZES)
    wrong = {k: (v, WS_SIZES[k]) for k, v in got.items() if v != WS_SIZES[k]}
    assert not wrong, wrong


# entry -> (size export, its arguments, the entry's arguments): placeholder pointers (16:
# aligned for every entry), "ws" / "nb" where the workspace and its byte count go. Valid small
# shapes whose workspace is not empty; the check runs before any launch. (Were a check to let
# one of these calls through, it would launch on the placeholder pointers: on a machine with a
# GPU that is a fault there, which is how a regression of a refusal would show.)
_P = 16
WS_ENTRIES = {
    "rpst_adain": ("adain", (2, 3), (_P, _P, _P, 2, 3, 16, 1e-5, "ws", "nb", None)),
    "rpst_mean_variance_norm": ("adain", (2, 3), (_P, _P, 2, 3, 16, 1e-5, "ws", "nb", None)),
    "rpst_masked_adain_params": ("masked_adain", (2, 3), (_P, _P, _P, _P, _P, 2, 3, 16, 12, 1e-5,
                                                          _P, "ws", "nb", None)),
    "rpst_conv2d_ws": ("conv2d", (2, 256, 37, 70, 96, 3, 4),
                       (_P, _P, _P, None, None, _P, 2, 256, 37, 70, 96, 3, 0, 4, 1, "ws", "nb",
                        None)),
    "rpst_conv2d_stats": ("conv2d_stats", (2, 128, 37, 200, 256, 3, 0),
                          (_P, None, _P, None, None, _P, 2, 128, 37, 200, 256, 3, 0, 0, 1, _P, _P,
                           1e-5, "ws", "nb", None)),
    "rpst_conv2d_stats_store": ("conv2d_stats", (2, 128, 37, 200, 256, 3, 0),
                                (_P, None, _P, None, None, _P, 2, 128, 37, 200, 256, 3, 0, 0, 1,
                                 _P, _P, 1e-5, 1, "ws", "nb", None)),
    "rpst_conv2d_gated": ("conv2d_gated", (2, 32, 16, 16, 32, 1),
                          (_P, _P, None, _P, _P, _P, 2, 32, 16, 16, 32, 1, _P, _P, 1e-5, "ws",
                           "nb", None)),
    "rpst_conv2d_mix": ("conv2d_mix", (2, 8, 9, 13, 32, 3),
                        (_P, _P, _P, _P, None, _P, 2, 8, 9, 13, 32, 3, 0, 1, "ws", "nb", None)),
    "rpst_resized_mean_std": ("resized_mean_std", (5, 7),
                              (_P, _P, _P, 2, 3, 5, 7, 10, 14, 1e-5, "ws", "nb", None)),
    "rpst_sanet_attention": ("sanet_attention", (2, 48),
                             (_P, _P, _P, _P, 2, 24, 48, "ws", "nb", None)),
    "rpst_cosine_affinity": ("cosine_affinity", (2, 24, 48),
                             (_P, _P, _P, 2, 24, 48, "ws", "nb", None)),
    "rpst_aea_clamp": ("aea_clamp", (2, 48, 16),
                       (_P, _P, _P, _P, _P, _P, 16, 0, 50.0, 0.0, 1.0, _P, _P, 2, 48, "ws", "nb",
                        None)),
    "rpst_adaptive_attention": ("adaptive_attention", (2, 24, 48, 16),
                                (_P, _P, _P, _P, _P, _P, _P, _P, _P, 16, 1, 50.0, 0.0, 1.0, _P,
                                 None, None, None, 2, 24, 48, "ws", "nb", None)),
    "rpst_sanet_attention_backward": ("sanet_attention_backward", (2, 48, 40),
                                      (_P, _P, _P, _P, _P, _P, _P, 2, 64, 48, 40, "ws", "nb",
                                       None)),
    "rpst_sanet_attention_backward_chunked": ("sanet_attention_backward_chunked", (2, 64, 48, 40),
                                              (_P, _P, _P, _P, _P, _P, _P, 2, 64, 48, 40, "ws",
                                               "nb", None)),
    "rpst_adaptive_attention_backward": ("adaptive_attention_backward", (2, 64, 48, 16),
                                         (_P, _P, _P, _P, _P, _P, _P, _P, _P, 16, 0, 50.0, 0.0,
                                          1.0, _P, _P, _P, _P, _P, _P, _P, _P, 2, 64, 48, "ws",
                                          "nb", None)),
    "rpst_conv1x1_wgrad": ("conv1x1_wgrad", (2, 100, 300),
                           (_P, _P, _P, _P, 2, 100, 48, 300, "ws", "nb", None)),
    "rpst_reflect_pad_border_grad": ("reflect_pad_border_grad", (2, 3, 5, 7),
                                     (_P, _P, _P, 2, 3, 16, 5, 7, "ws", "nb", None)),
    "rpst_reflect_pad_border_grad_masked": ("reflect_pad_border_grad", (2, 3, 5, 7),
                                            (_P, _P, None, _P, 2, 3, 16, 5, 7, "ws", "nb", None)),
    "rpst_conv_wgrad": ("conv_wgrad", (2, 16, 9, 13, 32),
                        (_P, _P, _P, _P, 2, 16, 9, 13, 32, "ws", "nb", None)),
    "rpst_conv_wgrad_pad": ("conv_wgrad", (2, 16, 9, 13, 32),
                            (_P, _P, _P, _P, 2, 16, 9, 13, 32, 1, "ws", "nb", None)),
    "rpst_conv7_wgrad": ("conv7_wgrad", (2, 3, 9, 13, 16),
                         (_P, _P, _P, _P, 2, 3, 9, 13, 16, 1, "ws", "nb", None)),
    # no size export: two floats per plane
    "rpst_adain_backward": (None, 2 * 6 * 4, (_P, _P, _P, _P, _P, _P, 6, 16, "ws", "nb", None)),
    "rpst_sq_diff_sum": ("sq_diff", (), (_P, _P, 100, 0.01, _P, "ws", "nb", None)),
    "rpst_wct_fuse": ("wct", (2, 16, 64), (_P, _P, _P, 2, 16, 64, None, "ws", "nb", None)),
    "rpst_wct_params": ("wct", (2, 16, 64),
                        (_P, _P, None, _P, _P, 2, 16, 64, None, "ws", "nb", None)),
    "rpst_whiten_and_color_f64": ("wct", (1, 16, 64), (_P, _P, _P, 16, 64, None, "ws", "nb",
                                                       None)),
    "rpst_whiten_and_color_original_f64": ("wct", (1, 16, 64),
                                           (_P, _P, _P, 16, 64, "ws", "nb", None)),
    "rpst_matrix_power_psd_f64": ("matrix_power", (16, 2),
                                  (_P, _P, 16, 2, 0, None, "ws", "nb", None)),
}


def _refusals(lib):
    """{(entry, "short" | "null"): (status, rpst_last_error())}: the workspace one byte short,
    then null with the full byte count."""
    out = {}
    for entry, (size, size_args, args) in WS_ENTRIES.items():
        need = size_args if size is None else _size_export(lib, size)(*size_args)
        assert need > 1, entry
        for defect, ws, nb in (("short", _P, need - 1), ("null", None, need)):
            call = tuple({"ws": ws, "nb": nb}.get(a, a) if isinstance(a, str) else a for a in args)
            status = getattr(lib, entry)(*call)
            out[(entry, defect)] = (status, lib.rpst_last_error().decode())
    return out


WS_REFUSALS = {('rpst_adain', 'short'): (-3, 'adain: workspace 95 < 96 bytes'),
 ('rpst_adain', 'null'): (-3, 'adain: workspace 96 < 96 bytes'),
 ('rpst_mean_variance_norm', 'short'): (-3, 'mean_variance_norm: workspace too small'),
 ('rpst_mean_variance_norm', 'null'): (-3, 'mean_variance_norm: workspace too small'),
 ('rpst_masked_adain_params', 'short'): (-3,
                                         'masked_adain_params: workspace 786431 < 786432 bytes '
                                         '(or unaligned)'),
 ('rpst_masked_adain_params', 'null'): (-3,
                                        'masked_adain_params: workspace 786432 < 786432 bytes '
                                        '(or unaligned)'),
 ('rpst_conv2d_ws', 'short'): (-3, 'conv2d: workspace 11213575 < 11213576 bytes'),
 ('rpst_conv2d_ws', 'null'): (-3, 'conv2d: workspace 11213576 < 11213576 bytes'),
 ('rpst_conv2d_stats', 'short'): (-3, 'conv2d_stats: workspace 196607 < 196608 bytes'),
 ('rpst_conv2d_stats', 'null'): (-3, 'conv2d_stats: workspace 196608 < 196608 bytes'),
 ('rpst_conv2d_stats_store', 'short'): (-3, 'conv2d_stats: workspace 196607 < 196608 bytes'),
 ('rpst_conv2d_stats_store', 'null'): (-3, 'conv2d_stats: workspace 196608 < 196608 bytes'),
 ('rpst_conv2d_gated', 'short'): (-3, 'conv2d_gated: workspace 2047 < 2048 bytes'),
 ('rpst_conv2d_gated', 'null'): (-3, 'conv2d_gated: workspace 2048 < 2048 bytes'),
 ('rpst_conv2d_mix', 'short'): (-3, 'conv2d_mix: workspace 8639 < 8640 bytes'),
 ('rpst_conv2d_mix', 'null'): (-3, 'conv2d_mix: workspace 8640 < 8640 bytes'),
 ('rpst_resized_mean_std', 'short'): (-3, 'resized_mean_std: workspace 47 < 48 bytes'),
 ('rpst_resized_mean_std', 'null'): (-3, 'resized_mean_std: workspace 48 < 48 bytes'),
 ('rpst_sanet_attention', 'short'): (-3, 'sanet_attention: workspace 19199 < 19200 bytes'),
 ('rpst_sanet_attention', 'null'): (-3, 'sanet_attention: workspace 19200 < 19200 bytes'),
 ('rpst_cosine_affinity', 'short'): (-3, 'cosine_affinity: workspace too small'),
 ('rpst_cosine_affinity', 'null'): (-3, 'cosine_affinity: workspace too small'),
 ('rpst_aea_clamp', 'short'): (-3, 'aea_clamp: workspace too small'),
 ('rpst_aea_clamp', 'null'): (-3, 'aea_clamp: workspace too small'),
 ('rpst_adaptive_attention', 'short'): (-3, 'adaptive_attention: workspace 45695 < 45696 bytes'),
 ('rpst_adaptive_attention', 'null'): (-3, 'adaptive_attention: workspace 45696 < 45696 bytes'),
 ('rpst_sanet_attention_backward', 'short'): (-3,
                                              'sanet_attention_backward: workspace too small'),
 ('rpst_sanet_attention_backward', 'null'): (-3, 'sanet_attention_backward: workspace too small'),
 ('rpst_sanet_attention_backward_chunked', 'short'): (-3,
                                                      'sanet_attention_backward_chunked: '
                                                      'workspace too small'),
 ('rpst_sanet_attention_backward_chunked', 'null'): (-3,
                                                     'sanet_attention_backward_chunked: '
                                                     'workspace too small'),
 ('rpst_adaptive_attention_backward', 'short'): (-3,
                                                 'adaptive_attention_backward: workspace too '
                                                 'small'),
 ('rpst_adaptive_attention_backward', 'null'): (-3,
                                                'adaptive_attention_backward: workspace too '
                                                'small'),
 ('rpst_conv1x1_wgrad', 'short'): (-3, 'conv1x1_wgrad: workspace too small'),
 ('rpst_conv1x1_wgrad', 'null'): (-3, 'conv1x1_wgrad: workspace too small'),
 ('rpst_reflect_pad_border_grad', 'short'): (-3, 'reflect_border_grad: workspace too small'),
 ('rpst_reflect_pad_border_grad', 'null'): (-3, 'reflect_border_grad: workspace too small'),
 ('rpst_reflect_pad_border_grad_masked', 'short'): (-3,
                                                    'reflect_border_grad: workspace too small'),
 ('rpst_reflect_pad_border_grad_masked', 'null'): (-3,
                                                   'reflect_border_grad: workspace too small'),
 ('rpst_conv_wgrad', 'short'): (-3, 'conv_wgrad: workspace too small'),
 ('rpst_conv_wgrad', 'null'): (-3, 'conv_wgrad: workspace too small'),
 ('rpst_conv_wgrad_pad', 'short'): (-3, 'conv_wgrad: workspace too small'),
 ('rpst_conv_wgrad_pad', 'null'): (-3, 'conv_wgrad: workspace too small'),
 ('rpst_conv7_wgrad', 'short'): (-3, 'conv7_wgrad: workspace too small'),
 ('rpst_conv7_wgrad', 'null'): (-3, 'conv7_wgrad: workspace too small'),
 ('rpst_adain_backward', 'short'): (-3, 'adain_backward: workspace too small'),
 ('rpst_adain_backward', 'null'): (-3, 'adain_backward: workspace too small'),
 ('rpst_sq_diff_sum', 'short'): (-3, 'sq_diff_sum: workspace too small'),
 ('rpst_sq_diff_sum', 'null'): (-3, 'sq_diff_sum: workspace too small'),
 ('rpst_wct_fuse', 'short'): (-3, 'wct_fuse: workspace 717239 < 717240 bytes'),
 ('rpst_wct_fuse', 'null'): (-3, 'wct_fuse: workspace 717240 < 717240 bytes'),
 ('rpst_wct_params', 'short'): (-3, 'wct_params: workspace 717239 < 717240 bytes'),
 ('rpst_wct_params', 'null'): (-3, 'wct_params: workspace 717240 < 717240 bytes'),
 ('rpst_whiten_and_color_f64', 'short'): (-3, 'whiten_and_color: workspace too small'),
 ('rpst_whiten_and_color_f64', 'null'): (-3, 'whiten_and_color: workspace too small'),
 ('rpst_whiten_and_color_original_f64', 'short'): (-3,
                                                   'whiten_and_color(original): workspace too '
                                                   'small'),
 ('rpst_whiten_and_color_original_f64', 'null'): (-3,
                                                  'whiten_and_color(original): workspace too '
                                                  'small'),
 ('rpst_matrix_power_psd_f64', 'short'): (-3, 'matrix_power: workspace too small'),
 ('rpst_matrix_power_psd_f64', 'null'): (-3, 'matrix_power: workspace too small')}


def test_workspace_one_byte_short_is_refused(monkeypatch):
    """Every entry point that takes a workspace refuses one that is a byte short, and a null
    one, with RPST_EWORKSPACE (-3) and its own message, before any launch (no GPU needed)."""
    for k in SIZE_ENV:
        monkeypatch.delenv(k, raising=False)
    got = _refusals(_lib.load())
    assert all(status == -3 for status, _ in WS_REFUSALS.values())
    assert got == WS_REFUSALS

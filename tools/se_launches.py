"""One SE block, `--calls` times, for a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/se_launches.py): per call the trace should hold two direct conv launches (conv1 and the
gated conv3), one F(4x4) conv (conv2), two statistics merges, one se_gate_kernel, and no
elementwise, pooling or reduction kernel. The first (warm-up) call also folds and packs the
weights."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rp-style-transfer_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=4, default=[2, 32, 512, 512])
    a = ap.parse_args()
    import network as net
    from rpst import ops, synth
    dev = torch.device("cuda:0")
    n, c, h, w = a.shape
    blk = net.Conv2dBlock(3, c, 3, 1, padding=1, attention="se")
    synth.synth_module_(torch.nn.ModuleList([blk]), 5)
    se = blk.attention_block.eval().to(dev)
    x = torch.from_numpy(synth.image(1, (n, c, h, w))).to(dev)
    with torch.no_grad():
        ops.se_bottleneck(x, se, stats=True)
        torch.cuda.synchronize()
        for _ in range(a.calls):
            ops.se_bottleneck(x, se, stats=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()

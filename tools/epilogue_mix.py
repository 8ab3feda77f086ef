"""Executed-path instruction mix of the position-quarter F(4x4) kernel's epilogue, per co tile
and wave, from a device .s file (hipcc -S --cuda-device-only with the Makefile's flags):

    python tools/epilogue_mix.py rpst_wino4q.s 'wino4q_mfma_kernelILi0ELb1ELb0ELb1E' [body]

The epilogue of quarter body `body` (0-3, default 0) runs from the accumulator fence (the
`s_nop 7` statement) to the run of 144 v_mov that zeroes the accumulators. The path counted is
the one an interior full-tile block on the buffer-store path takes: of all paths through the
epilogue's branches, the shortest that issues the 16 buffer_store_dwordx4; exec-mask branches
(s_cbranch_execz / execnz) fall through, backward branches are not taken. Regions are split at
s_barrier; the 12 regions are six exchange passes (write | read + first transform), the third
and sixth read region also holding two channels' second transform and finish.

Parts: `exchange` = the LDS traffic, barriers and waits of the pass regions and the exchange
reads of the two long regions; `transform` = the two passes of at6, taken as their arithmetic
(10 VALU per call, 24 + 16 calls: 400; the compiler sinks the first pass into the long regions
too, so it cannot be told from the statistics' adds by opcode); `other` = the rest: context,
bias, activation, statistics, store addressing and the stores.
"""
import collections
import sys

BR_UNIFORM = ("s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz")
AT6 = ("v_add_f32", "v_sub_f32", "v_fma_f32", "v_fmac_f32")


def kernel_lines(path, sym):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines)
                 if l.startswith("_Z") and sym in l and l.split(";")[0].rstrip().endswith(":"))
    out = []
    for l in lines[start + 1:]:
        if "s_endpgm" in l:
            break
        t = l.split(";")[0].strip()
        if t and not t.startswith("."):
            out.append(t)
        elif t.startswith(".LBB") and t.endswith(":"):
            out.append(t)
    return out


def cls(ins):
    op = ins.split()[0]
    if op in ("v_readlane_b32", "v_writelane_b32"):
        return "lane"
    if op == "v_readfirstlane_b32":
        return "readfirstlane"
    if op.startswith("ds_"):
        return "LDS"
    if op == "s_barrier":
        return "barrier"
    if op.startswith(("buffer_store", "global_store", "flat_store")):
        return "store"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    if op in ("s_nop", "s_waitcnt") or op.startswith(("s_cbranch", "s_branch")):
        return "wait/nop/branch"
    if op.startswith("v_"):
        return "at6?" if op.split("_e")[0] in AT6 or op in AT6 else "VALU"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def main():
    path, sym = sys.argv[1], sys.argv[2]
    body = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    L = kernel_lines(path, sym)
    label = {l[:-1]: i for i, l in enumerate(L) if l.endswith(":")}
    starts = [i for i, l in enumerate(L) if l.startswith("s_nop 7")]
    start = starts[body]
    # the 144 accumulators are zeroed by a run of v_mov (one v_mov 0 per tuple, then copies)
    ismov = [l.startswith("v_mov_b32_e32 v") for l in L]
    end = next(i for i in range(start, len(L) - 144) if ismov[i] and sum(ismov[i:i + 144]) >= 140)
    # shortest path start -> end over states (pc, buffer stores issued so far); a path that
    # reaches an MFMA has left the epilogue
    import heapq
    heap, seen, prev = [(0, start, 0)], set(), {}
    goal = None
    while heap:
        cost, pc, k = heapq.heappop(heap)
        if (pc, k) in seen:
            continue
        seen.add((pc, k))
        if pc == end:
            if goal is None or k > goal[1]:
                goal = (pc, k, cost)
            if k == 16:
                break
            continue
        ins = L[pc]
        op = ins.split()[0]
        if "mfma" in op or pc + 1 >= len(L):
            continue
        step = 0 if ins.endswith(":") else 1
        succ = [pc + 1]
        if op == "s_branch":
            succ = [label[ins.split()[1]]]
        elif op in BR_UNIFORM:
            succ.append(label[ins.split()[1]])
        k2 = k + (1 if op.startswith("buffer_store") else 0)
        for t in succ:
            if (t, k2) not in seen:
                if (t, k2) not in prev or prev[(t, k2)][0] > cost + step:
                    prev[(t, k2)] = (cost + step, pc, k)
                heapq.heappush(heap, (cost + step, t, k2))
    nst, tot = goal[1], goal[2]
    path, st = [], (end, nst)
    while st != (start, 0):
        _, pc, k = prev[st]
        path.append(pc)
        st = (pc, k)
    regs = [collections.Counter()]
    for pc in reversed(path):
        if L[pc].endswith(":"):
            continue
        regs[-1][cls(L[pc])] += 1
        if L[pc].split()[0] == "s_barrier":
            regs.append(collections.Counter())
    print(f"{sym} body {body}: lines {start}..{end}, path with {nst} buffer stores, {tot} instructions, "
          f"{len(regs)} regions")
    keys = ["VALU", "at6?", "readfirstlane", "SALU", "SMEM", "lane", "LDS", "barrier", "store", "vmem",
            "wait/nop/branch"]
    for i, r in enumerate(regs):
        print(f"  region {i:2d}: " + " ".join(f"{k}={r[k]}" for k in keys if r[k]))
    longs = sorted(range(len(regs)), key=lambda i: -sum(regs[i].values()))[:2]
    parts = {p: collections.Counter() for p in ("exchange", "transform", "other")}
    parts["transform"]["VALU"] = 400
    parts["other"]["VALU"] = -400
    for i, r in enumerate(regs):
        for k in keys:
            if k == "at6?":
                parts["other"]["VALU"] += r[k]
            elif i in longs and k != "barrier":
                parts["other"][k] += r[k]
            else:
                parts["exchange"][k] += r[k]
        if i in longs:  # the last pass's exchange reads open a long region
            ex = min(r["LDS"], 5)
            parts["other"]["LDS"] -= ex
            parts["exchange"]["LDS"] += ex
    for p, c in parts.items():
        print(f"  {p:9s}: " + " ".join(f"{k}={c[k]}" for k in keys if c[k]) + f"  total {sum(c.values())}")


if __name__ == "__main__":
    main()

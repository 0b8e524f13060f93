"""Tail listing of the XCD-local GRU kernels (csrc/gru_xl.hip) from the compiler's assembly.

usage:  hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -S --cuda-device-only \
            gru_xl.hip -o gru_xl.s
        python scripts/xl_tail_audit.py gru_xl.s [label] [--list]

The tail of a recurrence step is everything between the step's last MFMA and its publish: the
settle (forward) or the last record's wait states (backward), the io waves' stores, the partial
writes, the reduction barrier, the gate math and the publish stores.  Every instruction of it
is on the dependent chain of the recurrence.

Per product instantiation (the traced ones carry stamp code and are skipped) the tool takes
the basic blocks a step can run between its last MFMA and the step loop's header -- every
wave's path: the io waves' stores and the publisher's are both in it -- and leaves out the cold
paths, the blocks that lead straight into a loop of their own (the poison fill, a re-poll).  It
prints counts of LDS reads and writes, s_waitcnt by counter, barriers, quarter-rate integer
multiplies, v_mov, 32-lane swaps, transcendental and fp64 instructions, s_nop, stores, and all
instructions; with --list the blocks themselves follow, in text order.  What runs behind the
publish store up to the loop's end (the backward's bias sums and row maximum) is part of the
region: the listing shows on which side of the store an instruction sits.  Static text, every
block counted once.  A tool, not a test.
"""
import re
import sys

from xl_reg_audit import demangle, functions

QUARTER = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mul_hi_i32", "v_mul_lo_i32", "v_mad_u64_u32",
           "v_mad_i64_i32")
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")


def blocks_of(body):
    """The function as basic blocks in text order: [label, header comment, instructions]; a
    block ends at a label or behind a branch."""
    blocks = [["<entry>", "", []]]
    for ln in body:
        s = ln.strip()
        m = re.match(r"^(\.LBB\w+):\s*(;.*)?$", s)
        if m:
            blocks.append([m.group(1), m.group(2) or "", []])
            continue
        if not s or s.startswith((";", ".")):
            continue
        blocks[-1][2].append(re.sub(r"\s+", " ", s))
        if re.match(r"^s_c?branch|^s_endpgm", s):
            blocks.append(["", blocks[-1][1], []])
    return blocks


def successors(blocks, at):
    """(fall-through block or None, branch target block or None) of block `at`"""
    index = {b[0]: i for i, b in enumerate(blocks) if b[0]}
    last = blocks[at][2][-1] if blocks[at][2] else ""
    m = re.match(r"^s_(c?)branch\w* (\.LBB\w+)", last)
    to = index.get(m.group(2)) if m else None
    through = at + 1 if at + 1 < len(blocks) and not last.startswith(("s_branch", "s_endpgm")) else None
    return through, to


def tail_of(body):
    """The blocks a step can run between its last MFMA and the step loop's header, in text
    order, cold paths left out: [(label, instructions)]"""
    blocks = blocks_of(body)
    mf = [i for i, b in enumerate(blocks) if any(s.startswith("v_mfma") for s in b[2])]
    if not mf:
        return []
    hdr = re.search(r"(?:Header=|Parent Loop )(BB\w+) Depth=1", blocks[mf[-1]][1])
    if not hdr:
        return []
    header = ".L" + hdr.group(1)
    inner = lambda i: "Parent Loop" in blocks[i][1]
    in_loop = lambda i: hdr.group(1) in blocks[i][1]

    def cold(i):
        """straight on from block i (conditional branches fall through) an inner loop comes
        before a barrier, a publish store or the header: the poison fill or a re-poll"""
        for _ in range(12):
            if i is None or not in_loop(i) or blocks[i][0] == header:
                return False
            if inner(i):
                return True
            if any(s.startswith(("s_barrier", "buffer_store")) for s in blocks[i][2]):
                return False
            through, to = successors(blocks, i)
            i = through if through is not None else to
        return False

    keep, todo = set(), [mf[-1]]
    while todo:
        i = todo.pop()
        if i in keep:
            continue
        keep.add(i)
        for j in successors(blocks, i):
            if j is not None and in_loop(j) and blocks[j][0] != header and not cold(j):
                todo.append(j)
    out = []
    for i in sorted(keep):
        ins = blocks[i][2]
        if i == mf[-1]:   # behind the step's last MFMA
            ins = ins[max(k for k, s in enumerate(ins) if s.startswith("v_mfma")) + 1:]
        out.append((blocks[i][0], ins))
    return out


def counts(tail):
    code = [s for _, ins in tail for s in ins]
    c = {"instructions": len(code)}
    c["ds_read"] = sum(s.startswith("ds_read") for s in code)
    c["ds_write"] = sum(s.startswith("ds_write") for s in code)
    for k in ("vmcnt", "lgkmcnt", "expcnt"):
        c[f"s_waitcnt {k}"] = sum(s.startswith("s_waitcnt") and k in s for s in code)
    c["s_barrier"] = sum(s.startswith("s_barrier") for s in code)
    c["quarter-rate int mul"] = sum(s.startswith(QUARTER) for s in code)
    c["v_mov"] = sum(s.startswith("v_mov_") for s in code)
    c["v_permlane32_swap"] = sum(s.startswith("v_permlane32_swap") for s in code)
    c["transcendental"] = sum(s.startswith(TRANS) for s in code)
    c["fp64"] = sum(re.match(r"^v_\w+_f64", s) is not None for s in code)
    c["s_nop"] = sum(s.startswith("s_nop") for s in code)
    c["global/buffer store"] = sum(s.startswith(("global_store", "buffer_store")) for s in code)
    return c


def main():
    args = [a for a in sys.argv[1:] if a != "--list"]
    listing = "--list" in sys.argv
    path = args[0]
    label = args[1] if len(args) > 1 else path
    fns = {k: v for k, v in functions(open(path).read().split("\n")).items() if "xl_kernel" in k}
    nice = demangle(sorted(fns))
    print(f"== {label}: from the last MFMA of a step to the end of the step loop")
    for k in sorted(fns, key=lambda n: nice[n]):
        short = re.sub(r"^void ds2::|\(.*$", "", nice[k])
        # TRACE: the forward's second template argument, the backward's third
        pat = r"<\d+, true" if "fwd" in short else r"<\d+, \w+, true"
        if re.search(pat, short):
            continue
        tail = tail_of(fns[k])
        print(f"{short}:")
        print("  " + ", ".join(f"{a} {b}" for a, b in counts(tail).items()))
        if listing:
            for lab, ins in tail:
                if lab:
                    print(f"  {lab}:")
                for s in ins:
                    print("    " + s)


if __name__ == "__main__":
    main()

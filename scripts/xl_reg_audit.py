"""Register audit of the XCD-local GRU kernels (csrc/gru_xl.hip) from the compiler's assembly.

usage:  hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -S --cuda-device-only \
            gru_xl.hip -o gru_xl.s
        python scripts/xl_reg_audit.py gru_xl.s [label]

Per gru_{fwd,bwd}_xl_kernel instantiation it prints the kernel descriptor's vgpr_count (arch +
acc), agpr_count, sgpr_spill_count, vgpr_spill_count and scratch bytes, and the static counts of
copy / reload instructions inside the step loop: the outermost loop that holds the kernel's
MFMAs (from the earliest label in front of the first MFMA that a branch behind the last MFMA
jumps back to, up to that branch).  Static counts: timeout and re-poll paths inside the loop are
counted too, so they are an upper bound of what a step without a timeout executes.  A tool, not
a test."""
import re
import subprocess
import sys

COUNTED = ["v_mfma", "v_accvgpr_read", "v_accvgpr_write", "v_accvgpr_mov", "v_readlane",
           "v_writelane", "v_mov_b32", "v_mov_b64", "scratch_", "s_nop"]


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt"):
        try:
            out = subprocess.run([tool] + names, capture_output=True, text=True,
                                 check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def functions(lines):
    """name -> list of body lines (label line to .Lfunc_end)"""
    out, cur, name = {}, None, None
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
            else:
                cur.append(ln)
    return out


def metadata(lines):
    """kernel name -> dict of the amdhsa.kernels metadata fields"""
    out, cur = {}, {}
    for ln in lines:
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)\s*$", ln)
        if not m:
            continue
        k, v = m.groups()
        if k == "agpr_count" and "name" in cur:   # first key of a kernel's record
            cur = {}
        cur[k] = v
        if k == "name":
            out[v] = cur
        if k == "wavefront_size":                  # last key of a kernel's record
            if "name" in cur:
                out[cur["name"]] = cur
            cur = {}
    return out


def step_loop(body):
    ins = [(i, ln.strip()) for i, ln in enumerate(body)]
    mf = [i for i, s in ins if s.startswith("v_mfma")]
    if not mf:
        return body
    labels = {m.group(1): i for i, s in ins for m in [re.match(r"^(\.LBB\w+):", s)] if m}
    head, tail = None, None
    for i, s in ins:
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\w+)", s)
        if m and i > mf[-1] and labels.get(m.group(1), 1 << 30) < mf[0]:
            if head is None or labels[m.group(1)] < head:
                head, tail = labels[m.group(1)], i
    if head is None:
        return body[mf[0]:]
    return body[head:tail + 1]


def main():
    path = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 else path
    lines = open(path).read().split("\n")
    fns = {k: v for k, v in functions(lines).items() if "xl_kernel" in k}
    md = metadata(lines)
    nice = demangle(sorted(fns))
    print(f"== {label}")
    for k in sorted(fns, key=lambda n: nice[n]):
        d = md.get(k, {})
        short = re.sub(r"^void ds2::|\(.*$", "", nice[k])
        print(f"{short}: vgpr_count {d.get('vgpr_count')} agpr_count {d.get('agpr_count')} "
              f"sgpr_count {d.get('sgpr_count')} sgpr_spill_count {d.get('sgpr_spill_count')} "
              f"vgpr_spill_count {d.get('vgpr_spill_count')} "
              f"scratch_bytes {d.get('private_segment_fixed_size')}")
        loop = [ln.strip() for ln in step_loop(fns[k])]
        cnt = {c: sum(1 for s in loop if s.startswith(c)) for c in COUNTED}
        print("  step loop: " + ", ".join(f"{c} {n}" for c, n in cnt.items()))


if __name__ == "__main__":
    main()

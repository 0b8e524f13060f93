"""Per-kernel comparison of two builds' device assembly: which kernels one side has and the
other has not, and whether every kernel both have is the same code with the same resources.

usage:  hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only conv.hip -o before/conv.s
        hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only conv.hip -o after/conv.s   (etc.)
        python scripts/kernel_diff.py --before before/conv.s --after after/conv.s after/conv_split.s

Several files per side are one set of kernels (a source file split in two).  Per kernel name it
compares the function body (label to .Lfunc_end) and the amdhsa.kernels metadata record, after
replacing the compiler's function-local label numbers (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>): they
count functions and temporaries of the translation unit, so they move when a kernel moves.
Prints one line per kernel with the vgpr / agpr / sgpr / spill / scratch / LDS fields of the
`after` side and exits 1 when a common kernel differs.  A tool, not a test."""
import argparse
import re
import subprocess
import sys

FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size"]


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        try:
            out = subprocess.run([tool] + names, capture_output=True, text=True,
                                 check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def normalise(body):
    tmp = {}
    out = []
    for ln in body:
        ln = re.sub(r"(\.L|\b)BB\d+_", r"\1BB_", ln)   # .LBB<n>_<block>; BB<n>_<block> in comments
        ln = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln)
        ln = re.sub(r"\.Ltmp\d+", lambda m: tmp.setdefault(m.group(0), ".Ltmp%d" % len(tmp)), ln)
        out.append(re.sub(r"\s+", " ", ln).rstrip())   # comment columns follow the label width
    return out


def bodies(lines):
    """kernel name -> normalised body lines (label line to .Lfunc_end)"""
    out, cur, name = {}, None, None
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                out[name] = normalise(cur)
                cur = None
            else:
                cur.append(ln)
    return out


def records(lines):
    """kernel name -> the lines of its amdhsa.kernels record"""
    out = {}
    try:
        i = next(k for k, ln in enumerate(lines) if ln.startswith("amdhsa.kernels:")) + 1
    except StopIteration:
        return out
    rec = []
    for ln in lines[i:] + ["end"]:
        if ln.startswith("  - ") or not ln.startswith(" "):
            if rec:
                name = next(r.split()[-1] for r in rec if r.strip().startswith(".name:"))
                out[name] = [("    " + r[4:] if r.startswith("  - ") else r).rstrip() for r in rec]
            rec = []
            if not ln.startswith(" "):
                break
        rec.append(ln)
    return out


def load(paths):
    body, rec = {}, {}
    for p in paths:
        with open(p) as f:
            lines = f.read().split("\n")
        r = records(lines)
        b = bodies(lines)
        for name in r:            # kernels only: device functions have no record
            if name in rec:
                sys.exit(f"{name} is defined in two files of one side")
            rec[name], body[name] = r[name], b[name]
    return body, rec


def fields(rec):
    vals = {}
    for ln in rec:
        parts = ln.split()
        if len(parts) == 2 and parts[0].rstrip(":") in FIELDS:
            vals[parts[0].rstrip(":")] = parts[1]
    return " ".join(f"{f[1:]}={vals.get(f, '?')}" for f in FIELDS)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    args = ap.parse_args()
    b_body, b_rec = load(args.before)
    a_body, a_rec = load(args.after)
    names = sorted(set(b_rec) | set(a_rec))
    pretty = demangle(names)
    only_b = [n for n in names if n not in a_rec]
    only_a = [n for n in names if n not in b_rec]
    differ = []
    print(f"kernels: before {len(b_rec)}, after {len(a_rec)}, common {len(names) - len(only_b) - len(only_a)}")
    for n in names:
        if n in only_b:
            print(f"REMOVED    {pretty[n]}\n           {len(b_body[n])} lines; {fields(b_rec[n])}")
            continue
        if n in only_a:
            print(f"ADDED      {pretty[n]}\n           {len(a_body[n])} lines; {fields(a_rec[n])}")
            continue
        what = [w for w, same in (("code", b_body[n] == a_body[n]), ("metadata", b_rec[n] == a_rec[n]))
                if not same]
        if what:
            differ.append(n)
        print(f"{'DIFFERS' if what else 'identical':10s} {pretty[n]}\n           "
              f"{len(a_body[n])} lines; {fields(a_rec[n])}" +
              (f"\n           differs in {', '.join(what)}; before: {len(b_body[n])} lines; "
               f"{fields(b_rec[n])}" if what else ""))
    print(f"removed {len(only_b)}, added {len(only_a)}, differing {len(differ)}, "
          f"identical {len(names) - len(only_b) - len(only_a) - len(differ)}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

"""Compare two device assembly listings of one source file kernel by kernel: which kernels keep their machine code.

  hipcc <the Makefile's FLAGS> -x hip --cuda-device-only -S fdcm_exhaustive.hip -o new.s     (and the same on the parent: old.s)
  python tools/asm_kernel_diff.py old.s new.s

A kernel is its instructions and labels between its entry label and its end label; comments, directives and the kernel
descriptor (kernarg size, names) are left out, basic-block labels lose the function's number (.LBB12_3 -> .LBB_3), and a
kernel is matched by its mangled name up to --cut (a regular expression; what follows its first match is dropped, for a
parameter that was added at the end).  Prints SAME / DIFF / NEW / GONE per kernel; exit status 1 when a kernel differs or
is gone."""
import argparse
import re
import sys


def kernels(path, cut):
    out, cur, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            out[re.sub(cut + ".*$", "", cur) if cut else cur] = body
            cur = None
            continue
        s = ln.split(";")[0].rstrip()
        if s.strip() and not s.strip().startswith("."):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
        elif re.match(r"^\.LBB\d+_\d+:", s):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--cut", default="", help="regular expression: the mangled names are compared up to its first match")
    a = ap.parse_args()
    old, new = kernels(a.old, a.cut), kernels(a.new, a.cut)
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old:
            print("NEW ", len(new[k]), k)
        elif k not in new:
            print("GONE", len(old[k]), k)
            bad = 1
        else:
            same = old[k] == new[k]
            bad |= not same
            print("SAME" if same else "DIFF", len(old[k]), k)
    return bad


if __name__ == "__main__":
    sys.exit(main())

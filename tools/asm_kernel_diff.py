"""Compare two device assembly listings of one source file kernel by kernel: which kernels keep their machine code.

  hipcc <the Makefile's FLAGS> -x hip --cuda-device-only -S fdcm_exhaustive.hip -o new.s     (and the same on the parent: old.s)
  python tools/asm_kernel_diff.py old.s new.s

A kernel is its instructions and labels between its entry label and its end label; comments, directives and the kernel
descriptor (kernarg size, names) are left out, basic-block labels lose the function's number (.LBB12_3 -> .LBB_3), and a
kernel is matched by its mangled name up to --cut (a regular expression; what follows its first match is dropped, for a
parameter that was added at the end).  Prints SAME / DIFF / NEW / GONE per kernel; exit status 1 when a kernel differs or
is gone.

--rename PATTERN REPLACEMENT (may be repeated): an old kernel whose mangled name matches the regular expression is compared
with the new kernel of the name re.sub gives, the kernel that replaces it.  Such a pair prints as PAIR with, old -> new, its
instruction count and its registers, LDS and scratch from the kernel descriptor, and then every opcode whose count differs.
A pair is expected to differ: it sets the exit status only when the new kernel needs more VGPRs, SGPRs, LDS or scratch.

  python tools/asm_kernel_diff.py old.s new.s --rename 'k_nms_list_roundE.*' 'k_nms_roundILb1ELb0ELb0EEEvNS0_7NmsArgsE'"""
import argparse
import collections
import re
import sys

FIGURES = {"vgpr": "next_free_vgpr", "sgpr": "next_free_sgpr", "lds": "group_segment_fixed_size", "scratch": "private_segment_fixed_size"}


def kernels(path, cut):
    """name -> (body lines, {figure: value})"""
    out, cur, body, fig = {}, None, [], {}
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            cur, body, fig = m.group(1), [], {}
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            out[re.sub(cut + ".*$", "", cur) if cut else cur] = (body, fig)
            cur = None
            continue
        s = ln.split(";")[0].rstrip()
        m = re.match(r"^\s*\.amdhsa_(\w+)\s+(\d+)", s)
        if m:
            fig.update({k: int(m.group(2)) for k, v in FIGURES.items() if v == m.group(1)})
        if s.strip() and not s.strip().startswith("."):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
        elif re.match(r"^\.LBB\d+_\d+:", s):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def opcodes(body):
    return collections.Counter(ln.split()[0] for ln in body if not ln.endswith(":"))


def pair(old_name, new_name, old, new):
    """Prints the figures of a renamed kernel and of the one it replaces; True when a resource grew."""
    (ob, of), (nb, nf) = old, new
    oc, nc = opcodes(ob), opcodes(nb)
    print("PAIR", old_name, "->", new_name)
    print("     instructions %d -> %d" % (sum(oc.values()), sum(nc.values())),
          " ".join("%s %s -> %s" % (k, of.get(k, "?"), nf.get(k, "?")) for k in FIGURES))
    for op in sorted(set(oc) | set(nc)):
        if oc[op] != nc[op]:
            print("     %-28s %d -> %d" % (op, oc[op], nc[op]))
    return any(nf.get(k, 0) > of.get(k, 0) for k in FIGURES)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--cut", default="", help="regular expression: the mangled names are compared up to its first match")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("PATTERN", "REPLACEMENT"),
                    help="an old kernel whose name matches PATTERN is compared with the new kernel re.sub names")
    a = ap.parse_args()
    old, new = kernels(a.old, a.cut), kernels(a.new, a.cut)
    bad = 0
    paired = {}  # new name -> old name
    for k in sorted(old):
        for pat, rep in a.rename:
            k2 = re.sub(pat, rep, k)
            if k2 != k and k2 in new and k not in new:
                paired[k2] = k
                break
    for k in sorted(set(old) | set(new)):
        if k in paired.values():
            continue
        if k in paired:
            bad |= pair(paired[k], k, old[paired[k]], new[k])
        elif k not in old:
            print("NEW ", len(new[k][0]), k)
        elif k not in new:
            print("GONE", len(old[k][0]), k)
            bad = 1
        else:
            same = old[k][0] == new[k][0]
            bad |= not same
            print("SAME" if same else "DIFF", len(old[k][0]), k)
    return bad


if __name__ == "__main__":
    sys.exit(main())

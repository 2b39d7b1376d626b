"""Do two sets of device assemblies hold the same kernels under (possibly) other names?

    hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 --cuda-device-only -S anirec_train.hip -o OLD.s   (on the parent)
    ... the same on the change, once per translation unit the parent's file became ...   -o NEW_<unit>.s
    python scripts/isa_twins.py OLD.s NEW_train.s NEW_train_head.s ...

Splits each file by function symbol, drops comments and directives, renumbers local labels, and pairs every kernel of
OLD with a kernel of the NEW files (taken together: a kernel lives in one of them) that has the same instruction text
AND the same .amdhsa_ resources (VGPRs, SGPRs, accumulator offset, LDS and scratch bytes).  Device functions that are not
kernels (a noinline slow path) are compared too: a NEW file may hold its own copy of one, and EVERY copy must have the
instruction text and the register / scratch counts of OLD's function of that name.  Bodies are compared whole, as
opaque text.  Prints the old -> new name map of the kernels whose name changed, every kernel and function left without
a counterpart, and one result line; exit status 1 if any is left.
"""
import collections
import re
import subprocess
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
             "private_segment_fixed_size")
FUNC_RESOURCES = ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size")


def functions(path):
    """({kernel: (instruction text, resources)}, {other device function: (instruction text, resources)}) of one file."""
    lines = open(path).read().splitlines()
    kernel_names = {m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m}
    names = {m.group(1) for ln in lines for m in [re.match(r"\s*\.type\s+(\S+),@function", ln)] if m} | kernel_names
    body, res, cur = collections.defaultdict(list), collections.defaultdict(dict), None
    for ln in lines:
        ln = re.sub(r"\s*(;|//).*", "", ln).strip()
        m = re.match(r"(\S+):$", ln)
        if m and m.group(1) in names:
            cur = m.group(1)
        elif ln.startswith(".amdhsa_kernel"):
            cur = ln.split()[1] + "#desc"
        elif ln.startswith(".end_amdhsa_kernel") or ln.startswith(".Lfunc_end"):
            cur = None
        elif cur and cur.endswith("#desc"):
            m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", ln)
            if m and m.group(1) in RESOURCES:
                res[cur[:-5]][m.group(1)] = m.group(2)
        elif cur and ln and (not ln.startswith(".") or ln.startswith(".L")):
            body[cur].append(ln)
        else:  # what a function that is no kernel needs: .set [.L]<name>.<resource>, <value>
            m = re.match(r"\.set\s+(?:\.L)?(\S+)\.(\w+),\s*(.+)$", ln)
            if m and m.group(1) in names - kernel_names and m.group(2) in FUNC_RESOURCES:
                res[m.group(1)][m.group(2)] = m.group(3)
    out = ({}, {})
    for k in names:
        labels = {}
        text = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), "\n".join(body[k]))
        out[0 if k in kernel_names else 1][k] = (text, tuple(sorted(res[k].items())))
    return out


def demangle(names):
    if not names:
        return {}
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(old_path, new_paths):
    old, old_funcs = functions(old_path)
    new, copies, bad = {}, [], []  # copies: (file, name, code) of every device function of the NEW files
    for p in new_paths:
        ks, fs = functions(p)
        bad += ["  TWICE in %s: %s (also in an earlier file)" % (p, k) for k in ks if k in new]
        new.update(ks)
        copies += [(p, k, fs[k]) for k in sorted(fs)]
    by_code = collections.defaultdict(list)
    for k in sorted(new):
        by_code[new[k]].append(k)
    pairs, old_left = [], []
    for k in sorted(old):
        cands = by_code[old[k]]
        if k in cands:          # the same name first, so that identical bodies under two names pair up straight
            cands.remove(k)
            pairs.append((k, k))
        else:
            old_left.append(k)
    for k in list(old_left):
        if by_code[old[k]]:
            pairs.append((k, by_code[old[k]].pop(0)))
            old_left.remove(k)
    new_left = sorted(k for ks in by_code.values() for k in ks)
    func_bad = [(p, k) for p, k, code in copies if old_funcs.get(k) != code]
    func_lost = sorted(set(old_funcs) - {k for _, k, _ in copies})
    dm = demangle([n for p in pairs if p[0] != p[1] for n in p] + old_left + new_left + func_lost +
                  [k for _, k in func_bad])
    for o, n in pairs:
        if o != n:
            print("  %s  ->  %s" % (dm[o], dm[n]))
    for ln in bad:
        print(ln)
    for k in old_left:
        print("  UNMATCHED in %s: %s" % (old_path, dm[k]))
    for k in new_left:
        print("  UNMATCHED in NEW: %s" % dm[k])
    for k in func_lost:
        print("  DEVICE FUNCTION of %s in no NEW file: %s" % (old_path, dm[k]))
    for p, k in func_bad:
        print("  DEVICE FUNCTION of %s differs from (or is not in) %s: %s" % (p, old_path, dm[k]))
    print("%s vs %s: %d / %d kernels, %d matched (%d renamed), %d + %d unmatched; %d device functions, %d copies, "
          "%d equal" % (old_path, " ".join(new_paths), len(old), len(new), len(pairs), sum(o != n for o, n in pairs),
                        len(old_left), len(new_left), len(old_funcs), len(copies), len(copies) - len(func_bad)))
    return 1 if old_left or new_left or len(old) != len(new) or bad or func_bad or func_lost else 0


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2:]))

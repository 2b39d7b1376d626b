"""Do two device assemblies hold the same kernels under (possibly) other names?

    hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 --cuda-device-only -S anirec_train.hip -o OLD.s   (on the parent)
    ... the same on the change ...                                               -o NEW.s
    python scripts/isa_twins.py OLD.s NEW.s

Splits each file by kernel symbol, drops comments and directives, renumbers local labels, and pairs every kernel with a
kernel of the other file that has the same instruction text AND the same .amdhsa_ resources (VGPRs, SGPRs, accumulator
offset, LDS and scratch bytes).  Bodies are compared whole, as opaque text.  Prints the old -> new name map of the
kernels whose name changed, every kernel left without a counterpart, and one result line; exit status 1 if any is left.
"""
import collections
import re
import subprocess
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
             "private_segment_fixed_size")


def kernels(path):
    """{symbol: (instruction text, resources)} of one assembly file."""
    lines = open(path).read().splitlines()
    names = {m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m}
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
    out = {}
    for k in names:
        labels = {}
        text = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), "\n".join(body[k]))
        out[k] = (text, tuple(sorted(res[k].items())))
    return out


def demangle(names):
    if not names:
        return {}
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
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
    dm = demangle([n for p in pairs if p[0] != p[1] for n in p] + old_left + new_left)
    for o, n in pairs:
        if o != n:
            print("  %s  ->  %s" % (dm[o], dm[n]))
    for k in old_left:
        print("  UNMATCHED in %s: %s" % (old_path, dm[k]))
    for k in new_left:
        print("  UNMATCHED in %s: %s" % (new_path, dm[k]))
    print("%s vs %s: %d / %d kernels, %d matched (%d renamed), %d + %d unmatched"
          % (old_path, new_path, len(old), len(new), len(pairs), sum(o != n for o, n in pairs), len(old_left),
             len(new_left)))
    return 1 if old_left or new_left or len(old) != len(new) else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

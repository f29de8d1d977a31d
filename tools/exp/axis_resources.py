"""Registers, scratch, LDS and code size of every build of the (instance, axis)-per-lane solver (copra_lmpc_axis*), read from the code objects
of a built libcopra_hip.so: the table of profiles/OPTIMISATION_LOG.md for a change to lmpc_axis.hpp, one library against another.

    python tools/exp/axis_resources.py LIB [OTHER_LIB]        one row per kernel; with OTHER_LIB: both, and what differs

Needs llvm-objdump and llvm-readelf of ROCm; no GPU."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def resources(so_path, prefix="copra_lmpc_axis"):
    """kernel name -> dict(vgpr: architectural (the metadata's count less the AGPRs), agpr, sgpr, scratch, lds, code: bytes)"""
    out = {}
    with tempfile.TemporaryDirectory(prefix="copra_res_") as tmp:
        local = os.path.join(tmp, "lib.so")
        with open(so_path, "rb") as f, open(local, "wb") as g:
            g.write(f.read())
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=tmp, capture_output=True, text=True, check=True).stdout
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", f], cwd=tmp, capture_output=True, text=True, check=True).stdout
            size = {}
            for line in syms.splitlines():
                p = line.split()
                if len(p) >= 8 and p[3] == "FUNC":
                    size[p[7]] = int(p[2], 0) if not p[2].isdigit() else int(p[2])
            cur = {}
            for line in notes.splitlines():
                m = re.match(r"^\s*-?\s*(\.[a-z_]+):\s*(\S+)\s*$", line)
                if not m:
                    continue
                key, val = m.group(1), m.group(2)
                if line.startswith("  - "):  # (a kernel's record; the entries of its .args are indented further)
                    if prefix in cur.get(".name", ""):
                        _keep(out, cur, size)
                    cur = {}
                if line.startswith("    .") or line.startswith("  - "):
                    cur[key] = val
            if prefix in cur.get(".name", ""):
                _keep(out, cur, size)
    return out


def _keep(out, cur, size):
    if not all(k in cur for k in FIELDS):
        return
    out[cur[".name"]] = dict(vgpr=int(cur[".vgpr_count"]) - int(cur[".agpr_count"]), agpr=int(cur[".agpr_count"]), sgpr=int(cur[".sgpr_count"]),
                             scratch=int(cur[".private_segment_fixed_size"]), lds=int(cur[".group_segment_fixed_size"]), code=size.get(cur[".name"], -1))


def demangled(name):
    try:
        return subprocess.run([os.path.join(LLVM, "llvm-cxxfilt"), name], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return name


def main(argv):
    a = resources(argv[1])
    b = resources(argv[2]) if len(argv) > 2 else None
    cols = ("vgpr", "agpr", "sgpr", "scratch", "lds", "code")
    print("| kernel | " + " | ".join(cols) + " |")
    print("|---|" + "---|" * len(cols))
    for name in sorted(a):
        short = re.sub(r"^void |\(.*$", "", demangled(name))
        if b is None:
            print("| `%s` | %s |" % (short, " | ".join(str(a[name][c]) for c in cols)))
        else:
            o = b.get(name)
            print("| `%s` | %s |" % (short, " | ".join(("%d -> %d" % (a[name][c], o[c]) if o and o[c] != a[name][c] else str(a[name][c])) for c in cols)))
    if b is not None:
        worse = [n for n in a if n in b and b[n]["scratch"] > a[n]["scratch"]]
        print("\n%d kernels; scratch grows on %d" % (len(a), len(worse)))


if __name__ == "__main__":
    main(sys.argv)

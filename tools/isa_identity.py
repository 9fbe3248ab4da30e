#!/usr/bin/env python3
"""Whether two trees compile to the same kernels: `python tools/isa_identity.py PARENT_TREE NEW_TREE [unit ...]` compiles
every kernel unit (build.KERNEL_UNITS, or the units named) of both trees to assembly with the product's own flags
(build.HIPCC_FLAGS, as tools/isa_meta.py does), splits each output into kernels, normalises each kernel (normalise() below)
and compares, unit by unit, the multiset of (normalised instruction stream, register / spill / scratch / LDS figures of the
code object's metadata).  A kernel whose mangled name changed and nothing else pairs with its old self.  Prints per unit the
number of kernels, the number identical and every kernel of either side without a partner; exits non-zero if there is one.

It compares whole instruction streams and looks for no instruction in particular."""
import collections, os, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC_REL = os.path.join("ccv_mppi_path_tracker_amd", "csrc")
CXXFILT = "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
META_FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def normalise(text, symbol):
    """One kernel's assembly without what a renaming changes: comments stripped, directives other than .amdhsa_* dropped, local
    labels (.LBB0_3, ...) renumbered in order of first appearance, the kernel's own symbol replaced by a placeholder."""
    lines = []
    for line in text.replace(symbol, "KERNEL").splitlines():
        line = " ".join(line.split(";", 1)[0].split())
        if not line or (line.startswith(".") and not line.startswith(".amdhsa_") and not re.match(r"\.L\w+:$", line)):
            continue
        lines.append(line)
    labels = {}
    return re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), "\n".join(lines))


def split_kernels(asm):
    """{mangled name: its text from the entry label to the end of its kernel descriptor} of one assembly file"""
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel\n", asm, re.S | re.M):
        start = re.search(r"^%s:" % re.escape(m.group(1)), asm, re.M).start()
        out[m.group(1)] = asm[start:m.end()]
    return out


def metadata(asm):
    """{mangled name: META_FIELDS' values} from the file's .amdgpu_metadata"""
    out = {}
    for entry in re.split(r"^  - ", asm.split(".amdgpu_metadata", 1)[-1], flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if name:
            out[name.group(1)] = tuple(int(re.search(r"\.%s:\s+(\d+)" % f, entry).group(1)) for f in META_FIELDS)
    return out


def fingerprints(asm):
    """[(mangled name, (normalised text, metadata))] of every kernel of one assembly file"""
    meta = metadata(asm)
    return [(name, (normalise(text, name), meta[name])) for name, text in split_kernels(asm).items()]


def unpaired(parent, new):
    """the names of either side's kernels that have no partner with the same fingerprint on the other side"""
    left = collections.Counter(fp for _, fp in new)
    lone_parent = []
    for name, fp in parent:
        if left[fp] > 0:
            left[fp] -= 1
        else:
            lone_parent.append(name)
    lone_new = []
    for name, fp in new:
        if left[fp] > 0:
            left[fp] -= 1
            lone_new.append(name)
    return lone_parent, lone_new


def demangle(names):
    """by ROCm's llvm-cxxfilt, else a c++filt on the path, else the mangled names themselves"""
    tool = CXXFILT if os.path.exists(CXXFILT) else shutil.which("c++filt")
    if not names or not tool:
        return list(names)
    return subprocess.run([tool] + list(names), capture_output=True, text=True, check=True).stdout.splitlines()


def main():
    from ccv_mppi_path_tracker_amd import build
    trees = [os.path.abspath(t) for t in sys.argv[1:3]]
    units = [u if u.endswith(".hip") else u + ".hip" for u in sys.argv[3:]] or build.KERNEL_UNITS
    with tempfile.TemporaryDirectory() as tmp:
        def compile_one(job):
            side, unit = job
            out = os.path.join(tmp, "%d_%s.s" % (side, unit))
            subprocess.run([build.hipcc()] + build.HIPCC_FLAGS + ["-S", "--cuda-device-only", os.path.join(trees[side], CSRC_REL, unit), "-o", out],
                           check=True, stderr=subprocess.DEVNULL)
            with open(out) as f:
                fps = fingerprints(f.read())
            os.remove(out)
            return fps
        with ThreadPoolExecutor(8) as pool:
            results = list(pool.map(compile_one, [(side, unit) for unit in units for side in (0, 1)]))
    total = same = 0
    bad = False
    for i, unit in enumerate(units):
        parent, new = results[2 * i], results[2 * i + 1]
        lone_parent, lone_new = unpaired(parent, new)
        print("%-28s parent %3d  new %3d  identical %3d" % (unit, len(parent), len(new), len(parent) - len(lone_parent)))
        for side, names in (("parent", lone_parent), ("new", lone_new)):
            for name in demangle(names):
                print("    only in %s: %s" % (side, name))
        total += len(parent)
        same += len(parent) - len(lone_parent)
        bad = bad or lone_parent or lone_new or len(parent) != len(new)
    print("%d units: %d kernels in the parent, %d identical in the new tree" % (len(units), total, same))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Per-kernel resource metadata of the gfx950 code object inside libfiat_amd.so (build container or GPU box; needs only
the LLVM tools shipped with ROCm): name, VGPRs, AGPRs, SGPR / VGPR spills, private (scratch) bytes per lane, LDS.
`python tools/codeobject_report.py [--scratch]`; `kernels()` is used by tests/test_codeobject.py."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
LIB = os.path.join(ROOT, "fiat_amd", "csrc", "libfiat_amd.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(lib=LIB, all_units=False):
    """[{name, vgpr, agpr, sgpr_spill, vgpr_spill, scratch, lds, unit}] and the list of bundle targets in the library.  The
    library holds one code object per translation unit (unit: its position in the link line, 0 = api.hip); the default is
    api.hip's, the population tests/test_codeobject.py has set its budget on, ``all_units`` reads every one."""
    notes, listing = [], []
    with tempfile.TemporaryDirectory() as tmp:
        fat, one, dev = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "one.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib], check=True,
                       capture_output=True)
        # one bundle per translation unit (api.hip, wg.hip, bernstein.hip, hdivcurl.hip), back to back in the section:
        # the bundler reads the first one of a file only, so each is cut out and unbundled on its own
        with open(fat, "rb") as f:
            data = f.read()
        starts = [m.start() for m in re.finditer(BUNDLE_MAGIC, data)]
        for lo, hi in list(zip(starts, starts[1:] + [len(data)]))[:None if all_units else 1]:
            with open(one, "wb") as f:
                f.write(data[lo:hi])
            found = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o", f"--input={one}"],
                                   check=True, capture_output=True, text=True).stdout.split()
            listing += [t for t in found if t not in listing]
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={one}",
                            f"--targets={TARGET}", f"--output={dev}"], check=True, capture_output=True)
            notes.append(subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", dev], check=True, capture_output=True,
                                        text=True).stdout)
    out = []
    for unit, block in ((u, b) for u, text in enumerate(notes) for b in re.split(r"\n\s+- \.agpr_count:", text)[1:]):
        def num(key):
            m = re.search(rf"\.{key}:\s+(\d+)", block)
            return int(m.group(1)) if m else 0
        out.append({"name": re.search(r"\.name:\s+(\S+)", block).group(1), "agpr": int(block.split()[0]),
                    "vgpr": num("vgpr_count"), "sgpr_spill": num("sgpr_spill_count"), "vgpr_spill": num("vgpr_spill_count"),
                    "scratch": num("private_segment_fixed_size"), "lds": num("group_segment_fixed_size"), "unit": unit})
    return out, listing


def demangled(names):
    for tool in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
            if res.returncode == 0:
                return res.stdout.split("\n")
        except FileNotFoundError:
            pass
    return names


if __name__ == "__main__":
    ks, targets = kernels(all_units=True)
    print(f"{len(ks)} kernels, bundle targets: {targets}")
    only_scratch = "--scratch" in sys.argv
    ks = sorted(ks, key=lambda k: (-k["scratch"], -k["vgpr_spill"], k["name"]))
    names = demangled([k["name"] for k in ks])
    for k, n in zip(ks, names):
        if only_scratch and k["scratch"] == 0:
            continue
        print(f"scratch {k['scratch']:5d} B  vgpr {k['vgpr']:3d} agpr {k['agpr']:3d}  spills v{k['vgpr_spill']:4d} s{k['sgpr_spill']:4d}  {n[:150]}")

#!/usr/bin/env python3
"""Per-kernel resource usage of a built libsr_amd.so, from its code-object metadata (no GPU needed).

    python tools/kernel_resources.py lib/libsr_amd.so            # one line per kernel symbol
    python tools/kernel_resources.py OLD.so NEW.so               # compare: kernels of OLD must be unchanged in NEW

Every translation unit's device code sits in the library's .hip_fatbin section as one offload bundle; this
unbundles the gfx950 code object of each and reads the AMDGPU metadata note (VGPRs, AGPRs, SGPRs, spills,
scratch and static LDS bytes per kernel).  The comparison exits 1 when a kernel of OLD is missing from NEW
or differs in any of those figures; kernels only NEW has are listed.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(lib, arch="gfx950"):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat],
                       check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, s in enumerate(starts):
            piece = os.path.join(tmp, f"bundle{i}")
            with open(piece, "wb") as f:
                f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            co = os.path.join(tmp, f"co{i}")
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle",
                                f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--input={piece}", f"--output={co}"],
                               capture_output=True, text=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True,
                                   check=True).stdout
            cur = {}
            for line in notes.splitlines():
                m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(.*)$", line)
                if not m:
                    continue
                key, val = m.group(1), m.group(2).strip().strip("'\"")
                if line.lstrip().startswith("- ") and key != ".name" and cur.get(".symbol"):
                    cur = {}
                if key in FIELDS or key in (".name", ".symbol"):
                    if key == ".symbol" and ".symbol" in cur:
                        cur = {}
                    cur[key] = val
                if ".symbol" in cur and all(k in cur for k in FIELDS if k != ".agpr_count"):
                    out[cur[".symbol"]] = tuple(int(cur.get(k, 0)) for k in FIELDS)
    return out


def main(argv):
    if len(argv) == 2:
        for name, v in sorted(kernels(argv[1]).items()):
            print(name, *v)
        return 0
    if len(argv) != 3:
        print(__doc__)
        return 2
    old, new = kernels(argv[1]), kernels(argv[2])
    bad = 0
    for name, v in sorted(old.items()):
        if name not in new:
            print("MISSING", name)
            bad += 1
        elif new[name] != v:
            print("CHANGED", name, dict(zip(FIELDS, v)), "->", dict(zip(FIELDS, new[name])))
            bad += 1
    added = sorted(set(new) - set(old))
    print(f"{len(old)} kernels in {argv[1]}: {len(old) - bad} unchanged in {argv[2]}, {bad} missing or changed; "
          f"{len(added)} new")
    for name in added:
        print("NEW", name, *new[name])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

"""Static figures of the Gemma3 kernels (csrc/attn_gqa_wide.hip, csrc/gemma_kernels.hip) from the compiler's own resource-usage
remarks: compiles the two files with the Makefile's flags (the ones it adds for a single object included) plus
``-Rpass-analysis=kernel-resource-usage`` (objects go to a temporary directory) and writes profiles/gqa_wide_static.json.  Needs hipcc, no GPU.

    python tools/gqa_wide_static.py
"""
import json
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmlm_amd", "csrc")
FILES = ("attn_gqa_wide.hip", "gemma_kernels.hip")
FIELDS = (("sgpr", "TotalSGPRs"), ("vgpr", "VGPRs"), ("agpr", "AGPRs"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]"),
          ("waves_per_simd", r"Occupancy \[waves/SIMD\]"), ("sgpr_spill", "SGPRs Spill"), ("vgpr_spill", "VGPRs Spill"),
          ("static_lds_bytes", r"LDS Size \[bytes/block\]"))
# dynamic LDS is a launch argument the compiler does not see: Lds<T, 256>::BYTES of attn_wide.hpp = 2 tiles of 32 x (256 + pad)
# elements + the 16 KiB exchange area + 256 bytes of row constants
DYNAMIC_LDS = {"unsigned short": 2 * 32 * (256 + 8) * 2 + 16384 + 256, "float": 2 * 32 * (256 + 4) * 4 + 16384 + 256}


def _flags(src):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=(.*)$", mk, re.M).group(1).split()
    obj = "$(BUILD)/" + src[:-len(".hip")] + ".o"
    for targets, extra in re.findall(r"^(\$\(BUILD\)/.*?):\s*CXXFLAGS\s*\+=(.*)$", mk, re.M):
        if obj in targets.split():
            flags += extra.split()
    return [f.replace("$(ARCH)", "gfx950") for f in flags]


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")      # without one the mangled names are kept
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for src in FILES:
            err = subprocess.run([hipcc, *_flags(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, src + ".o")],
                                 cwd=CSRC, check=True, capture_output=True, text=True).stderr
            for block in re.split(r"remark: Function Name: ", err)[1:]:
                mangled = block.split()[0]
                name = subprocess.run([filt, mangled], check=True, capture_output=True, text=True).stdout.strip() if filt else mangled
                if "gqaw" not in name and "gemma_kernels" not in name:
                    continue
                name = re.sub(r"^void |\(.*$", "", name)
                row = {"kernel": name, "file": src}
                for key, pat in FIELDS:
                    row[key] = int(re.search(pat + r": (\d+)", block).group(1))
                if "gqaw::" in name and "delta" not in name:
                    row["dynamic_lds_bytes"] = DYNAMIC_LDS["float" if "<float" in name else "unsigned short"]
                rows.append(row)
    rows.sort(key=lambda r: r["kernel"])
    out = {"what": "registers, LDS and scratch of every kernel of attn_gqa_wide.hip and gemma_kernels.hip as hipcc's "
                   "-Rpass-analysis=kernel-resource-usage remarks report them (the Makefile's flags, gfx950); dynamic_lds_bytes is "
                   "the launch argument Lds<T, 256>::BYTES",
           "kernels": rows,
           "max_scratch_bytes_per_lane": max(r["scratch_bytes_per_lane"] for r in rows),
           "max_vgpr_spill": max(r["vgpr_spill"] for r in rows)}
    path = os.path.join(ROOT, "profiles", "gqa_wide_static.json")
    with open(path, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    for r in rows:
        print(f"{r['kernel']:110s} vgpr {r['vgpr']:3d} agpr {r['agpr']:3d} scratch {r['scratch_bytes_per_lane']} occ {r['waves_per_simd']}")
    assert out["max_scratch_bytes_per_lane"] == 0 and out["max_vgpr_spill"] == 0, "an instantiation uses scratch"


if __name__ == "__main__":
    main()

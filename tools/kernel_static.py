"""Static comparison of the gfx950 kernels of two builds of libgmlm_hip.so (no GPU needed): per kernel the symbol, the
VGPR count (AGPRs included), LDS bytes, scratch bytes, the number of v_mfma / scratch_ / packed-fp32 instructions, and
``body_sha1``: a hash of the disassembled instruction stream (mnemonics and operands; addresses, encodings and symbol offsets
stripped), from the code objects' metadata and disassembly.  Equal hashes = the same instructions in the same order.

    python tools/kernel_static.py --parent PARENT/libgmlm_hip.so --new gmlm_amd/libgmlm_hip.so \
        --match 'attn_|d128::' --added 'causal128::|rmsnorm_|qknorm_rope_|swiglu_' --out profiles/attn_causal_static.json

``--dynamic-lds 'REGEX=BYTES'`` (repeatable) records the dynamic LDS the host adds at launch for kernels whose static
``lds_bytes`` is not the whole picture.  ``--match``: kernels (demangled name, regex) that must be the same in both builds; ``--added``: kernels only the new build
has, listed with their figures.  ``--bare`` pairs the kernels by name without the parameter list, for a build in which a kernel's
parameter type moved namespace; a symbol of another length also moves the zero padding behind a kernel, which the disassembler
prints as a line "...", so with this flag that line is neither counted nor hashed: for a kernel that ends in padding,
``instructions`` is one less and ``body_sha1`` another than in a record made without the flag.  Exit status 1 when a matched
kernel differs or is missing.
"""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def code_objects(so, into):
    """The gfx950 ELF code objects embedded in the .so's offload bundles, one file each."""
    fat = os.path.join(into, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so, os.path.join(into, "so")],
                   check=True, capture_output=True)
    blob = open(fat, "rb").read()
    files, i = [], 0
    while True:
        i = blob.find(b"\x7fELF", i)
        if i < 0:
            return files
        shoff, = struct.unpack_from("<Q", blob, i + 0x28)
        shentsize, shnum = struct.unpack_from("<HH", blob, i + 0x3A)
        path = os.path.join(into, "co%d.o" % len(files))
        with open(path, "wb") as f:
            f.write(blob[i:i + shoff + shentsize * shnum])
        files.append(path)
        i += shoff + shentsize * shnum


def demangle(names):
    import torch                                               # the ROCm llvm tools ship no c++filt; torch carries a demangler
    return {n: torch._C._demangle(n) for n in names}


def kernels(so, skip_padding=False):
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(so, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            meta = {}
            for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                g = lambda key: re.search(r"\." + key + r":\s*(\S+)", blk)
                if g("name") and g("vgpr_count"):
                    meta[g("name").group(1)] = dict(vgpr=int(g("vgpr_count").group(1)), lds_bytes=int(g("group_segment_fixed_size").group(1)),
                                                    scratch_bytes=int(g("private_segment_fixed_size").group(1)))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                sym, body = m.group(1), m.group(2)
                if sym not in meta:
                    continue
                text = re.sub(r"//.*", "", body)                    # the comment holds the address, the encoding and <symbol+offset>
                if skip_padding:                                    # "...": zero padding up to the next symbol, layout and not code
                    text = re.sub(r"^\s*\.\.\.\s*$", "", text, flags=re.M)
                ops = re.findall(r"^\s*(\S+)", text, re.M)
                stream = "\n".join(" ".join(ln.split()) for ln in text.splitlines() if ln.strip())
                d = dict(meta[sym])
                d.update(v_mfma=sum(o.startswith("v_mfma") for o in ops), scratch_instr=sum(o.startswith("scratch_") for o in ops),
                         packed_f32=sum(bool(re.match(r"v_pk_\w+_f32", o)) for o in ops), instructions=len(ops),
                         body_sha1=hashlib.sha1(stream.encode()).hexdigest()[:16],
                         waves_per_simd=min(8, 512 // ((meta[sym]["vgpr"] + 7) // 8 * 8)) if meta[sym]["vgpr"] else 8)
                res[sym] = d
    names = demangle(list(res))
    return {re.sub(r"^void ", "", names[s]): dict(symbol=s, **d) for s, d in res.items()}


def bare(name):
    """The demangled name without its parameter list (template arguments kept)."""
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            name = name[:i]
            break
    # library templates (rocprim) run to a kilobyte: keep the head and a hash of the whole name
    return name if len(name) <= 120 else name[:96] + "...#" + hashlib.sha1(name.encode()).hexdigest()[:10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", required=True)
    ap.add_argument("--match", required=True)
    ap.add_argument("--added", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dynamic-lds", action="append", default=[], metavar="REGEX=BYTES",
                    help="dynamic LDS the host requests at launch for the kernels matching REGEX (lds_bytes is the static part only); "
                         "recorded as given")
    ap.add_argument("--compact", action="store_true", help="one short line per kernel (unchanged kernels: name and figures once)")
    ap.add_argument("--bare", action="store_true",
                    help="pair the kernels of the two builds by name without the parameter list (a parameter type that moved namespace)")
    a = ap.parse_args()
    old, new = kernels(a.parent, a.bare), kernels(a.new, a.bare)
    if a.bare:
        for ks in (old, new):
            assert len({bare(k) for k in ks}) == len(ks), "two kernels share a name without its parameter list"
        old, new = ({bare(k): dict(d, symbol=bare(k)) for k, d in ks.items()} for ks in (old, new))
    keys = ("symbol", "vgpr", "lds_bytes", "scratch_bytes", "v_mfma", "scratch_instr", "packed_f32", "instructions", "body_sha1")
    rows, bad = [], 0
    for name in sorted(k for k in old if re.search(a.match, k)):
        o, n = old[name], new.get(name)
        same = n is not None and all(o[k] == n[k] for k in keys)
        bad += not same
        rows.append(dict(kernel=name, parent={k: o[k] for k in keys[1:]}, new=None if n is None else {k: n[k] for k in keys[1:]},
                         unchanged=same))
    added = [dict(kernel=k, **{x: v for x, v in d.items() if x != "symbol"}) for k, d in sorted(new.items())
             if a.added and re.search(a.added, k) and k not in old]
    res = dict(what="per-kernel static figures of two builds of libgmlm_hip.so (same flags): vgpr = .vgpr_count + AGPRs as the code "
                    "object metadata reports it, instructions / v_mfma / scratch_instr / packed_f32 counted in the disassembly",
               match=a.match, compared=len(rows), unchanged=len(rows) - bad, existing=rows, added=added)
    dyn = {k: int(v) for k, v in (x.rsplit("=", 1) for x in a.dynamic_lds)}
    if dyn:
        res["dynamic_lds_bytes"] = dyn
    text = json.dumps(res, indent=1)
    if a.compact:
        # one line per kernel: [name without its parameter list, figures in the order of "columns"]; a changed kernel keeps its full row
        flat = [[bare(r["kernel"])] + [r["parent"][k] for k in keys[1:]] if r["unchanged"] else r for r in rows]
        extra = [k for k in (added[0] if added else {}) if k != "kernel" and k not in keys]
        new_rows = [[bare(d["kernel"])] + [d[k] for k in list(keys[1:]) + extra] for d in added]
        head = dict(what=res["what"], match=a.match, compared=len(rows), unchanged=len(rows) - bad,
                    columns=["kernel"] + list(keys[1:]), added_columns=["kernel"] + list(keys[1:]) + extra)
        if dyn:
            head["dynamic_lds_bytes"] = dyn
        lines = lambda xs: ",\n".join("  " + json.dumps(x) for x in xs)
        text = json.dumps(head)[:-1] + ',\n "existing": [\n' + lines(flat) + '\n ],\n "added": [\n' + lines(new_rows) + "\n ]}"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(f"{len(rows)} kernels compared, {len(rows) - bad} unchanged, {len(added)} added")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

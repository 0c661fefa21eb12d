"""Host contract of the twelve grouped streaming-attention entry points (gmlm_attention_causal_d128_*, _causal_d64_*,
_bidir_gqa_*; padded and packed, forward and backward), compared between two builds of libgmlm_hip.so without a GPU.

    python tools/attn_grouped_contract.py --parent PARENT/libgmlm_hip.so --new gmlm_amd/libgmlm_hip.so \
        --out profiles/attn_grouped_contract.json

Every call is made on fabricated addresses: without a device a refused call returns before any launch and a valid one ends in
GMLM_ELAUNCH, so the return code and the text of gmlm_last_error() show which check decided.  Each build makes the same calls
in a process of its own; the two lists of (code, message) must be equal byte for byte, but for the "(file:line)" that a failed
launch appends to its message: that names the launch statement in the source, which moves with the code, and is counted apart
(`launch_site_only`).  The calls: for each entry point and each of its valid baselines, the baseline itself, every argument set
to each value of VALUES (a superset of the single-argument mutations in tests/test_llama_cpu.py, tests/test_bidir_cpu.py and the
causal-d128 rows of tests/test_abi_contract_cpu.py), and the calls of PAIRS, which break two rules at once and so pin the order
of the checks.  Refuses to run where a device is present.  Exit status 1 when a call differs."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

A = 0x10000000                      # fabricated, non-null, 16-byte aligned
F32, BF16 = 0, 1

FWD = "q k v kv_len b hq hkv lq lk d q_stride k_stride v_stride scale dropout_p out out_lo lse dtype stream".split()
BWD = ("q k v out out_lo dout lse kv_len b hq hkv lq lk d q_stride k_stride v_stride scale dropout_p dq dk dv dq_stride dk_stride "
       "dv_stride dtype workspace workspace_bytes stream").split()
VFWD = "q k v cu_seqlens num_seqs max_len total_rows hq hkv d q_stride k_stride v_stride scale dropout_p out out_lo lse dtype stream".split()
VBWD = ("q k v out out_lo dout lse cu_seqlens num_seqs max_len total_rows hq hkv d q_stride k_stride v_stride scale dropout_p dq dk dv "
        "dq_stride dk_stride dv_stride dtype workspace workspace_bytes stream").split()
LISTS = {"fwd": FWD, "bwd": BWD, "varlen_fwd": VFWD, "varlen_bwd": VBWD}
POINTERS = "q k v kv_len out out_lo lse dout dq dk dv workspace cu_seqlens stream".split()
FLOATS = ("scale", "dropout_p")


def base(d, hq, hkv, **kw):
    w = {n + "_stride": (hq if n in ("q", "dq") else hkv) * d for n in ("q", "k", "v", "dq", "dk", "dv")}
    return dict(dict(q=A, k=A, v=A, kv_len=None, b=2, hq=hq, hkv=hkv, lq=64, lk=64, d=d, scale=0.125, dropout_p=0.0, out=A, out_lo=None,
                     lse=A, dtype=BF16, stream=None, dout=A, dq=A, dk=A, dv=A, workspace=A, workspace_bytes=1 << 40, cu_seqlens=A,
                     num_seqs=2, max_len=64, total_rows=100, **w), **kw)


# stem -> the valid baselines of the family (the shapes of the three test modules, and a loose-stride one)
FAMILIES = {
    "gmlm_attention_causal_d128": [base(128, 2, 1, b=1, lq=1, lk=1, num_seqs=1, max_len=1, total_rows=1, scale=0.088),
                                   base(128, 6, 2, q_stride=1280, k_stride=1280, v_stride=1280, dq_stride=1280, dk_stride=1280, dv_stride=1280)],
    "gmlm_attention_causal_d64": [base(64, 6, 2, q_stride=640, k_stride=640, v_stride=640, dq_stride=640, dk_stride=640, dv_stride=640),
                                  base(64, 2, 1, dtype=F32)],
    "gmlm_attention_bidir_gqa": [base(64, 6, 2, q_stride=640, k_stride=640, v_stride=640, dq_stride=640, dk_stride=640, dv_stride=640),
                                 base(128, 6, 2, q_stride=1280, k_stride=1280, v_stride=1280, dq_stride=1280, dk_stride=1280, dv_stride=1280),
                                 base(128, 4, 4, dtype=F32)],
}

BIG = (1 << 31) // 6 + 1
VALUES = dict(
    d=(0, 32, 64, 96, 128, 256), dtype=(F32, BF16, 2, -1), hq=(0, -1, 1, 2, 3, 7), hkv=(0, -1, 2, 3, 4), dropout_p=(-0.1, 0.1, 0.5, 1.0),
    scale=(0.0, -1.0), b=(-1, 0, 1 << 30, 1 << 40), lq=(0, 1, 63, 300, 1 << 30), lk=(0, 2, 65, 300), num_seqs=(-1, 0, 1 << 30, 1 << 40),
    max_len=(-1, 0, 1, 1 << 30, 1 << 40), total_rows=(-1, 0, 1, 1 << 30), workspace_bytes=(0, 1, 100 * 4 - 1, 2 * 6 * 64 * 4 - 1, 2 * 6 * 64 * 4),
    **{n + "_stride": (0, 56, 120, 128, 248, 260, 264, 376, 384, 392, 642, 644, 1284, (1 << 24) - 8, 1 << 24)
       for n in ("q", "k", "v", "dq", "dk", "dv")},
    **{p: (None, A + 2, A + 4, A + 8, A + 16) for p in POINTERS if p != "stream"})

# two rules broken at once: the first check in the order of attn_host.hpp decides
PAIRS = [dict(d=96, dtype=2), dict(d=32, dtype=-1), dict(hq=0, cu_seqlens=None), dict(b=-1, cu_seqlens=None), dict(hq=0, d=96),
         dict(dropout_p=0.5, scale=0.0), dict(dropout_p=-0.1, scale=-1.0), dict(b=BIG, lq=1, lk=1, q=None), dict(num_seqs=BIG, max_len=1, q=None),
         dict(b=BIG, lq=1, lk=1), dict(b=BIG - 2, lq=1, lk=1), dict(num_seqs=BIG, max_len=1), dict(num_seqs=BIG - 2, max_len=1),
         dict(q_stride=8, workspace_bytes=0), dict(dv_stride=8, workspace=None), dict(dq_stride=644, workspace_bytes=1),
         dict(lk=65, hq=7), dict(hq=7, dropout_p=0.1), dict(scale=0.0, lq=1 << 30, lk=1 << 30), dict(dtype=2, out_lo=A),
         dict(dtype=F32, out_lo=A, d=96), dict(out_lo=A + 8, lk=65), dict(max_len=0, total_rows=-1), dict(total_rows=1 << 30, d=96),
         dict(max_len=1 << 30, d=96), dict(num_seqs=1 << 30, dtype=2), dict(out=None, q_stride=8), dict(dout=None, workspace_bytes=0),
         dict(lse=None, dq=None), dict(b=0, d=96), dict(b=0, dropout_p=0.5), dict(lq=0, lk=0, q=None), dict(lq=0, lk=0, scale=0.0),
         dict(num_seqs=0, q=None), dict(total_rows=0, hq=7), dict(num_seqs=0, cu_seqlens=None), dict(b=0, q=None, k=None, v=None, out=None),
         dict(kv_len=A), dict(kv_len=A, b=-1), dict(out_lo=A), dict(out_lo=A, dtype=F32), dict(k=None, v=None)]


def calls():
    """[(function name, argument names, argument dict)] in a fixed order."""
    out = []
    for stem, bases in FAMILIES.items():
        for which, names in LISTS.items():
            for bs in bases:
                muts = [{}] + [{k: v} for k in names if k in VALUES for v in VALUES[k]] + [m for m in PAIRS if all(k in names for k in m)]
                out += [(stem + "_" + which, names, dict(bs, **m)) for m in muts]
    return out


def run(path):
    """Make every call on one build; prints [[code, message], ...] as JSON."""
    import torch
    assert torch.cuda.device_count() == 0, "fabricated addresses: never run this where a device is present"
    lib = C.CDLL(path)
    lib.gmlm_last_error.restype = C.c_char_p
    res = []
    for fn, names, a in calls():
        f = getattr(lib, fn)
        f.restype = C.c_int
        args = [C.c_void_p(a[n]) if n in POINTERS else C.c_float(a[n]) if n in FLOATS else C.c_int(a[n]) if n == "dtype"
                else C.c_size_t(a[n]) if n == "workspace_bytes" else C.c_int64(a[n]) for n in names]
        rc = f(*args)
        res.append([rc, lib.gmlm_last_error().decode("latin-1") if rc else ""])
    for stem in FAMILIES:                                   # the six size companions
        for fn, shapes in ((stem + "_workspace_bytes", [(2, 6, 300), (0, 6, 0), (1, 1, 1), (-1, 2, 3)]),
                           (stem + "_varlen_workspace_bytes", [(100, 6), (0, 6), (1, 1), (5, -1)])):
            f = getattr(lib, fn)
            f.restype = C.c_size_t
            res += [[f(*[C.c_int64(v) for v in s]), fn] for s in shapes]
    json.dump(res, sys.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--new")
    ap.add_argument("--out", default=None)
    ap.add_argument("--run", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run:
        return run(a.run)
    got = [json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--run", os.path.abspath(p)], check=True,
                                     capture_output=True, text=True).stdout) for p in (a.parent, a.new)]
    cs = calls()
    labels = [(fn, {k: v for k, v in args.items() if k in names}) for fn, names, args in cs]
    labels += [("workspace size", {})] * (len(got[0]) - len(cs))
    assert len(got[0]) == len(got[1]) == len(labels)
    site = lambda r: [r[0], re.sub(r" \([^()]*:\d+\)$", "", r[1]) if r[0] == -3 else r[1]]     # GMLM_ELAUNCH: "... (file:line)"
    differ = [dict(call=fn, args=args, parent=o, new=n) for (fn, args), o, n in zip(labels, *got) if site(o) != site(n)]
    site_only = sum(o != n and site(o) == site(n) for o, n in zip(*got))
    codes = {}
    for rc, _ in got[1][:len(cs)]:
        codes[str(rc)] = codes.get(str(rc), 0) + 1
    res = dict(what="return code and gmlm_last_error() text of the grouped streaming-attention entry points, parent build against new "
                    "build, on fabricated addresses without a device (tools/attn_grouped_contract.py)",
               entry_points=len(FAMILIES) * len(LISTS), calls=len(cs), size_calls=len(labels) - len(cs), return_codes_new=codes,
               distinct_messages=len({m for _, m in got[1][:len(cs)]}), launch_site_only=site_only, differ=differ)
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(f"{len(labels)} calls, {len(differ)} differ, {site_only} only in the launch site; codes {codes}")
    for d in differ[:20]:
        print(d)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()

"""Host side of the split-K weight-gradient kernel (no GPU needed): argument checks that reject before any launch, the
workspace plan, and a disassembly screen of the built gfx950 code objects for the new kernels."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

from gmlm_amd import _lib

LLVM = "/opt/rocm/llvm/bin"


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


def _call(lib, dy=16, ld_dy=768, x=16, ld_x=768, t=65536, n=768, k=768, splits=0, out=16, ld_out=768, flags=0, ws=16,
          ws_bytes=1 << 40):
    return lib.gmlm_wgrad_bf16(dy, ld_dy, x, ld_x, t, n, k, splits, out, ld_out, flags, ws, ws_bytes, None)


def test_wgrad_workspace_plan():
    lib = _lib_or_skip()
    # default plan: about one round of 256 workgroups (36 x 7, 27 x 9, 9 x 28 tiles x slices), capped by the 32-row stages
    assert lib.gmlm_wgrad_workspace_bytes(91712, 3072, 768, 0) == 7 * 3072 * 768 * 4
    assert lib.gmlm_wgrad_workspace_bytes(91712, 2304, 768, 0) == 9 * 2304 * 768 * 4
    assert lib.gmlm_wgrad_workspace_bytes(91712, 768, 768, 0) == 28 * 768 * 768 * 4
    assert lib.gmlm_wgrad_workspace_bytes(91712, 768, 768, 5) == 5 * 768 * 768 * 4
    assert lib.gmlm_wgrad_workspace_bytes(64, 256, 256, 0) == 2 * 256 * 256 * 4
    assert lib.gmlm_wgrad_workspace_bytes(16, 256, 256, 0) == 0
    assert lib.gmlm_wgrad_workspace_bytes(16384, 8192, 8192, 0) == 8192 * 8192 * 4     # 1024 tiles: one slice


@pytest.mark.parametrize("bad", [
    dict(dy=0), dict(x=0), dict(out=0), dict(ws=0),
    dict(n=96), dict(k=160), dict(n=0), dict(t=31),
    dict(ld_dy=700), dict(ld_x=767), dict(ld_out=770), dict(ld_dy=772),
    dict(dy=24), dict(x=8), dict(out=4), dict(ws=40),
    dict(splits=-1), dict(flags=6),
])
def test_wgrad_rejects_bad_arguments(bad):
    lib = _lib_or_skip()
    # GMLM_EINVAL, returned before anything is launched; a missing workspace is GMLM_EWORKSPACE like a short one
    assert _call(lib, **bad) == (-2 if bad == dict(ws=0) else -1)
    assert b"wgrad_bf16" in lib.gmlm_last_error()


def test_wgrad_rejects_small_workspace():
    lib = _lib_or_skip()
    need = lib.gmlm_wgrad_workspace_bytes(65536, 768, 768, 0)
    assert _call(lib, ws_bytes=need - 1) == -2           # GMLM_EWORKSPACE
    assert b"workspace" in lib.gmlm_last_error()


def _code_objects(so, into):
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


def test_wgrad_kernels_disassembly():
    """No packed-fp32 VALU in the new kernels (DESIGN.md section 5 b) and no scratch (spill) traffic."""
    _lib_or_skip()
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-objcopy"))):
        pytest.skip("ROCm llvm tools not found")
    tmp = tempfile.mkdtemp()
    try:
        bodies = {}
        for co in _code_objects(_lib.LIB_PATH, tmp):
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True,
                                 text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(_ZN4gmlm\d+wgrad_\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                bodies[m.group(1)] = m.group(2)
        names = sorted(bodies)
        assert any("wgrad_bf16_kernel" in n for n in names) and any("wgrad_combine_kernel" in n for n in names), names
        for name, body in bodies.items():
            assert "v_mfma" in body or "combine" in name
            for op in ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"):
                assert op not in body, (name, op)
            assert "scratch_" not in body and "buffer_store" not in body, name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

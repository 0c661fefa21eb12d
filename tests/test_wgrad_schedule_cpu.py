"""Host side of the two main-loop schedules of the split-K weight-gradient kernel (no GPU needed): the flag word, the
constant shared by the header and ops, and the two instantiations of the main kernel in the built library."""
import os
import re

import pytest

from gmlm_amd import _lib, ops

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmlm_hip.so not built")
    return _lib.lib()


@pytest.mark.parametrize("flags", [4, 5, 6, 7])
def test_wgrad_rejects_unknown_flag_bits(flags):
    lib = _lib_or_skip()
    # pointers that no kernel could use: the call has to return before anything is launched
    rc = lib.gmlm_wgrad_bf16(16, 768, 16, 768, 65536, 768, 768, 0, 16, 768, flags, 16, 1 << 40, None)
    assert rc == -1                                      # GMLM_EINVAL
    assert b"wgrad_bf16" in lib.gmlm_last_error() and b"flags" in lib.gmlm_last_error()


def test_wgrad_flag_constants_match_header():
    text = open(os.path.join(ROOT, "include", "gmlm_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(GMLM_WGRAD_\w+)\s+(\w+)\s*$", text, re.M)}
    assert defs == {"GMLM_WGRAD_NO_REMAP": ops.WGRAD_NO_REMAP, "GMLM_WGRAD_ONE_PHASE": ops.WGRAD_ONE_PHASE}
    assert ops.WGRAD_ONE_PHASE == 2 and ops.WGRAD_NO_REMAP == 1


def test_wgrad_library_holds_both_schedules():
    _lib_or_skip()
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(re.findall(rb"_ZN4gmlm\d+wgrad_bf16_kernel\w*", blob))
    assert len(names) == 2, names                        # the one-phase and the two-phase instantiation of one template

"""The inputs of tests/test_gpu_softmax_spikes.py do what its table claims (no GPU needed): ``softmax_trace`` replays the
kernels' schedule in float64 on every case's inputs after they are rounded to the case's dtype.

  * every planned jump is >= 7 log2 units against the reference the kernel holds, in a wave that already holds one, and the
    wave has rows that go through alpha = 1; every planned deferral is 4 - 5 units with no rescale of its wave in that tile,
    its second key >= 7 against the KEPT reference and < 6 against the row's true max; the window case has its late row;
  * the schedule with the rescale left out (alpha = 1 in O and l) misses the case's ``out`` budget by >= 10x in max-rel, and so
    does a reference that ignores the mask for any one masked spike: the inputs discriminate;
  * plain N(0, 1) inputs at every (head dim, key tile) in use rescale in no (wave, tile) step after a wave's first tile, which
    is why the GPU file exists;
  * every compiled streaming forward kernel is run by a spiked case here, by the older spike tests, or is listed in
    ``NOT_SPIKED`` with one of two reasons; stale entries fail;
  * the table is consistent: unique ids, lens, spikes inside their tensors, masked spikes masked for every query of their
    sequence."""
import re

import pytest
import torch

import test_gpu_attention_matrix as AM
import test_gpu_softmax_spikes as S
from test_attention_matrix_cpu import _compiled_kernels
from test_gpu_decoder_ops import TN

bf, f32 = torch.bfloat16, torch.float32
TRACED = [c for c in S.CASES if c.kind in ("jump", "table")]
IDS = lambda cs: [c.id for c in cs]

_TRACES = {}


def _trace(c, si=0):
    if (c.id, si) not in _TRACES:
        _TRACES[(c.id, si)] = S.seq_trace(c, S.inputs(c), si)
    return _TRACES[(c.id, si)]


def _heads(c, s):
    """the query heads a spike is aligned with"""
    if s["kind"] in ("table", "c2p"):
        return [0]
    if s["kind"] == "p2c":
        return [1 % c.hq]
    return [S._qhead(c, kh) for kh in range(c.hkv)]


@pytest.mark.parametrize("c", TRACED, ids=IDS(TRACED))
def test_planned_spikes_in_the_trace(c):
    tr, kt = _trace(c), c.kt
    plan = [s for s in S._plan(c) if s["seq"] == 0 and s["kind"] != "masked"]
    assert plan
    sc, mask, _ = S.seq_scores(c, S.inputs(c), 0)
    sc = (sc * S.LOG2E).masked_fill(~mask, -S.INF)
    mates_seen = 0
    for s in plan:
        i, t, w = s["i"], s["j"] // kt, s["i"] // 32
        for h in _heads(c, s):
            if s["kind"] == "table":
                # every query below n - 45 of head 0 meets the entry: rows that hold a reference jump by >= 7 in many waves
                hit = (tr.jump[h] >= S.JUMP_MIN) & tr.held[h] & torch.isfinite(tr.jump[h])
                assert int(hit.sum()) >= 32 and int(tr.after_first[h].sum()) >= 4, (int(hit.sum()), int(tr.after_first[h].sum()))
                continue
            j = float(tr.jump[h, i, t])
            print(f"  {c.id} {s['kind']} query {i} key {s['j']} (tile {t}) head {h}: jump {j:.2f} log2 units, wave rescales: "
                  f"{bool(tr.rescale[h, w, t])}")
            assert bool(tr.held[h, i, t]), "the row holds no reference yet: alpha would multiply zeros"
            mates = tr.held[h, w * 32:(w + 1) * 32, t] & (tr.alpha[h, w * 32:(w + 1) * 32, t] == 1.0)
            if s["kind"] == "defer" and s["step"] == 1:
                assert 4.0 <= j <= 5.0, j
                assert not bool(tr.rescale[h, w, t]), "a wave-mate rescales in the tile of the deferred key"
                assert c.seqs[0][1] >= (w + 1) * 32, "the deferred query sits in a partial wave"
                continue
            assert j >= S.JUMP_MIN and bool(tr.rescale[h, w, t]) and bool(tr.after_first[h, w, t]), j
            assert 0.0 < float(tr.alpha[h, i, t]) < 2.0 ** -S.JUMP_MIN
            mates_seen += int(mates.sum())
            if s["kind"] == "defer":
                true_max = float(sc[h, i, :t * kt].max())
                assert float(sc[h, i, s["j"]]) - true_max < S.K_DEFER, "against the true max this key would rescale as well"
            if s["kind"] == "late":
                late = s["late_row"]
                assert late // 32 == w and not bool(tr.held[h, late, t]) and float(tr.jump[h, late, t]) == S.INF
                assert bool(tr.rescale[h, w, :t].any()), "the wave has computed no tile before the late row meets its band"
                assert float(tr.alpha[h, late, t]) == 0.0
    assert c.kind == "table" or mates_seen >= 1, "no row of a rescaling wave goes through alpha = 1"


def _maxrel(a, b, rows):
    return float((a[rows] - b[rows]).abs().max()) / float(b[rows].abs().max())


@pytest.mark.parametrize("c", S.CASES, ids=IDS(S.CASES))
def test_own_scores_agree_with_the_family_reference(c):
    """``dense_out`` (this suite's scores and masks, which the trace reads) against the family's own float64 reference, and the
    trace's weights against both."""
    dat = S.inputs(c)
    own, ref = S.dense_out(c, dat), S.reference(c)["out"]
    assert float((own - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    if c.kind != "masked":
        traced = S.dense_out(c, dat, weights=lambda si: _trace(c, si).weights)
        assert float((traced - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


@pytest.mark.parametrize("c", TRACED, ids=IDS(TRACED))
def test_rescale_left_out_misses_the_budget(c):
    dat = S.inputs(c)
    r0, n, _ = c.seqs[0]
    wrong = S.dense_out(c, dat, weights=lambda si: _trace(c, si).weights_no_rescale)
    miss = _maxrel(wrong, S.reference(c)["out"], slice(r0, r0 + n))
    lim = S.family_budget(c, c.dtype, "out")[0]
    steps = sum(int(_trace(c, si).after_first.sum()) for si in range(len(c.seqs)))
    print(f"  {c.id}: alpha = 1 gives max|err| / max|ref| = {miss:.2e} (budget {lim:.0e}); {steps} (wave, tile) steps rescale after the first tile")
    assert miss >= 10 * lim, (miss, lim)


MASKED = [(c, i) for c in S.CASES for i, s in enumerate(S._plan(c)) if s["kind"] == "masked"]


@pytest.mark.parametrize("c,i", MASKED, ids=[f"{c.id}-{S._plan(c)[i]['pos']}" for c, i in MASKED])
def test_mask_ignored_misses_the_budget(c, i):
    dat, s = S.inputs(c), S._plan(c)[i]
    r0, n, nk = c.seqs[s["seq"]]
    key = c.seqs[s["kseq"]][0] + s["j"]
    foreign = [] if s["kseq"] == s["seq"] else [key]
    sc, mask, _ = S.seq_scores(c, dat, s["seq"], foreign)
    col = n if foreign else s["j"]
    if s["vbig"]:                                                  # a / d / e: no query of the sequence sees the key
        assert not bool(mask[:, col].any()), "the key is visible to some query of the sequence"
    assert not bool(mask[s["i"], col]), "the aligned query sees the key"
    for kh in range(c.hkv):
        h = S._qhead(c, kh)
        top = float(sc[h, s["i"]].masked_fill(~mask[s["i"]], -S.INF).max())
        assert top > -S.INF, "the aligned query sees no key at all"
        assert float(sc[h, s["i"], col]) - top >= S.MASK_MARGIN, (float(sc[h, s["i"], col]), top)
    wrong = S.dense_out(c, dat, unmask={s["seq"]: [key]})
    miss = _maxrel(wrong, S.reference(c)["out"], slice(r0, r0 + n))
    lim = S.family_budget(c, c.dtype, "out")[0]
    print(f"  {c.id} {s['pos']}: the mask ignored gives max|err| / max|ref| = {miss:.2e} (budget {lim:.0e})")
    assert miss >= 10 * lim, (miss, lim)


def test_random_inputs_never_rescale_after_the_first_tile():
    """The control: N(0, 1) q and k at every (head dim, key tile, mask) of the table, scale d^-0.5, two sequences of the table's
    lengths, 4 heads.  After a wave's first tile no (wave, tile) step rescales: the largest growth of a reference stays under 6."""
    seen = set()
    for c in TRACED:
        key = (c.d, c.kt, c.causal, c.window)
        if key in seen:
            continue
        seen.add(key)
        g = torch.Generator().manual_seed(c.d * 1000 + c.kt)
        steps = total = 0
        worst = 0.0
        for n in (200, 257):
            q, k = torch.randn(4, n, c.d, generator=g).to(c.dtype).double(), torch.randn(4, n, c.d, generator=g).to(c.dtype).double()
            sc = (q @ k.transpose(1, 2)) * c.d ** -0.5 * S.LOG2E        # unit-variance scores
            tr = S.softmax_trace(sc.masked_fill(~S._mask(c, n, n), -S.INF), c.kt)
            steps += int(tr.after_first.sum())
            total += int(tr.after_first.numel())
            grown = tr.jump[tr.held & torch.isfinite(tr.jump)]
            worst = max(worst, float(grown.max()))
        print(f"  d = {c.d}, kt = {c.kt}, causal {c.causal}, window {c.window}: {steps} of {total} steps rescale, largest growth {worst:.2f}")
        # the band is the exception: a row's first tile may hold a handful of keys, and rows of one wave meet their first key in
        # different tiles, so the window kernel does rescale on random data; every other family never does
        assert steps == 0 or c.window, key


# ------------------------------------------------------------------------------------------------ coverage of the code objects
FORWARD_PREFIXES = ("attn_fwd_kernel<", "attn_fwd_pipe_kernel<", "d128::fwd_kernel<", "d32::fwd_kernel<", "wide::fwd_kernel<",
                    "gqaw::fwd_kernel<", "gqa::causal64_fwd_kernel<", "causal128::fwd_kernel<", "bidir::gqa_fwd_kernel<",
                    "mbert::window_fwd_kernel<", "relb::fwd_kernel<", "disent::fwd_kernel<")
WAVES, DROP = "same body text, other wave count", "same body text, other DROP value"
_BOOL = ("false", "true")
NOT_SPIKED = {
    # attn_fwd_kernel<T, D, NW, DROP>: the older spike tests run fp32 d = 64 at 2 and 8 waves, d = 96 at 2 and 8, bf16 d = 64 at 2
    **{AM.fwd(AM.F32, d_, 4, False): WAVES for d_ in (64, 96)},
    AM.fwd(AM.BF, 64, 4, False): WAVES,
    **{AM.fwd(AM.F32, d_, nw, True): DROP for d_ in (64, 96) for nw in (2, 4, 8)},
    **{AM.fwd(AM.BF, 64, nw, True): DROP for nw in (2, 4)},
    # attn_fwd_pipe_kernel<D, NW, DROP, 2>: spiked at (64, 4), (96, 4), (96, 8)
    **{AM.pfwd(d_, nw, True): DROP for d_, nw in ((64, 4), (96, 4), (96, 8))},
    **{AM.d128("fwd", t, True): DROP for t in (AM.F32, AM.BF)},
    # d32::fwd_kernel<T, NW, DROP>: 1 wave is <= 32 rows (one key tile), 2 waves in bf16 are <= 128 rows (two 64-key tiles):
    # neither reaches a third tile, so no spike can follow a deferred one there
    **{f"d32::fwd_kernel<{t}, {nw}, {dr}>": WAVES for t, nws in ((AM.F32, (1,)), (AM.BF, (1, 2))) for nw in nws for dr in _BOOL},
    f"d32::fwd_kernel<{AM.F32}, 2, true>": DROP,
    **{f"wide::fwd_kernel<{t}, {d_}, true>": DROP for t in (AM.F32, AM.BF) for d_ in (384, 512)},
}
# the older spike tests: test_gpu_kernels.py (_RESCALE_FAMILIES and test_attention_online_softmax_rescale_branch) and
# test_gpu_decoder_ops.py (test_causal_attention_online_softmax_spikes_below_the_diagonal)
OLDER = {AM.fwd(AM.F32, 64, 2, False), AM.pfwd(64, 4, False)} | {f"causal128::fwd_kernel<{TN[t]}>" for t in (bf, f32)}


def _older():
    import test_gpu_kernels
    return OLDER | {v[6] for v in test_gpu_kernels._RESCALE_FAMILIES.values()}


def _sibling(name, reason):
    """the regular expression of the names that differ from ``name`` in the wave count / the DROP value alone"""
    if reason == DROP:
        return re.escape(name).replace("true", "false")
    args = name[name.index("<") + 1:-1].split(", ")
    at = 2 if name.startswith("attn_fwd_kernel<") else 1
    args = [re.escape(a) for a in args]
    args[at] = r"\d+"
    return re.escape(name[:name.index("<") + 1]) + ", ".join(args) + ">"


def test_every_streaming_forward_is_spiked_or_has_a_reason():
    compiled = _compiled_kernels(lambda n: n.startswith(FORWARD_PREFIXES))
    assert compiled, "no streaming forward kernel found in the code objects"
    unreachable = {n for n in AM.UNREACHABLE if n.startswith(FORWARD_PREFIXES)}    # no call can launch them, spiked or not
    spiked = set().union(*(c.fwd for c in TRACED)) | _older()
    listed = spiked | set(NOT_SPIKED) | unreachable
    assert not sorted(compiled - listed), f"compiled, but neither spiked nor in NOT_SPIKED: {sorted(compiled - listed)}"
    assert not sorted(listed - compiled), f"listed but not compiled: {sorted(listed - compiled)}"
    assert not sorted(spiked & set(NOT_SPIKED)), f"both spiked and in NOT_SPIKED: {sorted(spiked & set(NOT_SPIKED))}"
    for name, reason in NOT_SPIKED.items():
        assert reason in (WAVES, DROP), name
        pat = re.compile(_sibling(name, reason))
        twins = [n for n in spiked | {m for m, r_ in NOT_SPIKED.items() if r_ != reason} if n != name and pat.fullmatch(n)]
        assert twins, f"{name}: no spiked kernel differs from it in what '{reason}' names alone"
    for prefix in FORWARD_PREFIXES:                                # never a whole family
        assert any(n.startswith(prefix) for n in spiked), prefix


def test_case_table_is_consistent():
    ids = IDS(S.CASES)
    assert len(ids) == len(set(ids))
    for c in S.CASES:
        assert c.family in ("dense", "grouped", "window", "relb", "disent") and c.layout in ("padded", "packed"), c.id
        assert c.kind in ("jump", "table", "masked") and c.hq % c.hkv == 0 and c.kt in (32, 64), c.id
        assert (c.p > 0) == any(", true" in n for n in c.fwd | c.bwd if not n.startswith(("gqaw::", "gqas::"))), c.id
        assert all("fwd" in n for n in c.fwd) and not any("fwd" in n for n in c.bwd) and c.fwd and c.bwd, c.id
        if c.layout == "padded":
            assert c.l > 0 and all(0 <= n <= c.l for n in c.lens) and c.rows == c.l * len(c.lens), c.id
        else:
            assert c.l == 0 and sum(c.lens) == c.rows and c.seqs[-1][0] + c.seqs[-1][1] == c.rows, c.id
        n0 = c.seqs[0][1]
        if c.kind != "masked":
            assert -(-n0 // c.kt) >= 4 or (n0 == 104 and c.kt == 32), c.id           # >= 4 key tiles ...
            assert n0 % c.kt != 0, c.id                                             # ... the last one partial
        plan = S._plan(c)
        assert any(s["kind"] == "masked" for s in plan), c.id
        keys = set()
        for s in plan:
            qr0, qn, _ = c.seqs[s["seq"]]
            kr0, kn, _ = c.seqs[s["kseq"]]
            if s["kind"] != "table":
                assert 0 <= s["i"] < qn and 0 <= s["j"] < kn, (c.id, s)
                assert (kr0 + s["j"]) not in keys, (c.id, s, "two spikes on one key")
                keys.add(kr0 + s["j"])
            if s["kind"] == "masked":
                foreign = [] if s["kseq"] == s["seq"] else [kr0 + s["j"]]
                _, mask, _ = S.seq_scores(c, S.inputs(c), s["seq"], foreign)
                assert not bool(mask[:, qn if foreign else s["j"]].any()) or not s["vbig"], (c.id, s)
                assert bool(mask[s["i"]].any()), (c.id, s, "the aligned query sees nothing")
        dat = S.inputs(c)
        for t in (dat.q, dat.k, dat.v, dat.go):
            assert t.shape[0] == c.rows and torch.equal(t, t.to(c.dtype).float()), c.id     # values of the case's dtype


def test_print_rescale_steps_per_family():
    """Not a check: per family, how many (wave, tile) steps of its cases rescale after a wave's first tile (random inputs: 0)."""
    fam = {}
    for c in TRACED:
        key = c.id.split("_")[0]
        n = sum(int(_trace(c, si).after_first.sum()) for si in range(len(c.seqs)))
        fam[key] = fam.get(key, 0) + n
    for key, n in sorted(fam.items()):
        print(f"  {key}: {n}")
    assert all(n > 0 for n in fam.values())

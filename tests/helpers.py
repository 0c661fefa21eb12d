"""Shared test helpers: golden loading, oracle model construction from the parameter recipe, the float64 attention reference,
the restated dropout masks and the device kernel names a call launches."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    for k in ("config", "grad_norms"):
        if k in d:
            d[k] = json.loads(str(d[k]))
    return d


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bert_state_template(hidden, layers, inter, vocab, max_pos, pooler=True):
    """HF BertModel state-dict key -> shape, without instantiating transformers."""
    s = {"embeddings.word_embeddings.weight": (vocab, hidden),
         "embeddings.position_embeddings.weight": (max_pos, hidden),
         "embeddings.token_type_embeddings.weight": (2, hidden),
         "embeddings.LayerNorm.weight": (hidden,), "embeddings.LayerNorm.bias": (hidden,)}
    for i in range(layers):
        p = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            s[p + f"attention.self.{n}.weight"] = (hidden, hidden)
            s[p + f"attention.self.{n}.bias"] = (hidden,)
        s[p + "attention.output.dense.weight"] = (hidden, hidden)
        s[p + "attention.output.dense.bias"] = (hidden,)
        s[p + "attention.output.LayerNorm.weight"] = (hidden,)
        s[p + "attention.output.LayerNorm.bias"] = (hidden,)
        s[p + "intermediate.dense.weight"] = (inter, hidden)
        s[p + "intermediate.dense.bias"] = (inter,)
        s[p + "output.dense.weight"] = (hidden, inter)
        s[p + "output.dense.bias"] = (hidden,)
        s[p + "output.LayerNorm.weight"] = (hidden,)
        s[p + "output.LayerNorm.bias"] = (hidden,)
    if pooler:
        s["pooler.dense.weight"] = (hidden, hidden)
        s["pooler.dense.bias"] = (hidden,)
    return s


def model_state_template(f_in, hc, c, plm, num_relations=5, num_bases=30):
    """main.GraphTextLM state-dict key -> shape."""
    p = plm["hidden"]
    dims = [f_in, hc, 2 * hc, 4 * hc, 8 * hc]
    s = {"gnn_mask_token_embed": (1, f_in)}
    for k in range(4):
        s[f"rgcn{k+1}.weight"] = (num_bases, dims[k], dims[k + 1])
        s[f"rgcn{k+1}.comp"] = (num_relations, num_bases)
        s[f"rgcn{k+1}.root"] = (dims[k], dims[k + 1])
        s[f"rgcn{k+1}.bias"] = (dims[k + 1],)
        for n in ("weight", "bias", "mean_scale"):
            s[f"gnorm{k+1}.{n}"] = (dims[k + 1],)
    for k, (i, o) in enumerate(((f_in, hc), (hc, 2 * hc), (2 * hc, 8 * hc))):
        s[f"residual_proj{k+1}.weight"] = (o, i)
        s[f"residual_proj{k+1}.bias"] = (o,)
    for k, v in bert_state_template(p, plm["layers"], plm["inter"], plm["vocab"], plm["max_pos"]).items():
        s["plm_encoder." + k] = v
    s["multi_scale_fusion.scale_weights"] = (4,)
    for k in range(4):
        s[f"multi_scale_fusion.projections.{k}.weight"] = (p, dims[k + 1])
        s[f"multi_scale_fusion.projections.{k}.bias"] = (p,)
    s["multi_scale_fusion.layer_norm.weight"] = (p,)
    s["multi_scale_fusion.layer_norm.bias"] = (p,)
    for a in ("graph_to_text_attn", "text_to_graph_attn"):
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[f"{a}.{n}.weight"] = (p, p)
            s[f"{a}.{n}.bias"] = (p,)
    s["fusion_network.0.weight"] = (p, 2 * p)
    s["fusion_network.0.bias"] = (p,)
    s["fusion_network.1.weight"] = (p,)
    s["fusion_network.1.bias"] = (p,)
    s["classifier.0.weight"] = (hc, p)
    s["classifier.0.bias"] = (hc,)
    s["classifier.3.weight"] = (c, hc)
    s["classifier.3.bias"] = (c,)
    return s


def oracle_model_from_config(cfg):
    from gmlm_oracle import OracleGraphTextLM
    from param_recipe import recipe_state_dict
    plm = cfg["plm"]
    sd = recipe_state_dict(model_state_template(cfg["f_in"], cfg["hc"], cfg["c"], plm), cfg["seed"])
    plm_sd = {k[len("plm_encoder."):]: v for k, v in sd.items() if k.startswith("plm_encoder.")}
    m = OracleGraphTextLM(cfg["f_in"], cfg["hc"], cfg["c"], plm_sd, plm["heads"])
    m.load_reference_state(sd)
    return m, sd


def attn_dropout_scale(seed: int, slab: int, nq: int, nk: int, p: float, device="cpu"):
    """The attention kernels' replayable probability-dropout mask, restated with torch integer arithmetic (checker only;
    DESIGN.md section 4 'Dropout'): one 32-bit hash word per 2 x 2 (query, key) tile,
    word = lowbias32(base + (q >> 1) * C1 + (k >> 1) * C2), base = (lo32(seed) ^ hi32(seed)) + slab * C3, the element's 8-bit
    field = bits [16 (q & 1) + 8 (k & 1), +8), kept when field >= round(256 p); kept elements are scaled by 256 / (256 - th).
    ``slab`` = (batch * heads + head) * lq for padded tensors.  Returns the [nq, nk] float64 multiplier (0 or keep scale)."""
    m32 = 0xFFFFFFFF
    c1, c2, c3 = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D
    th = int(round(p * 256.0))
    th = max(0, min(255, th))
    ks = 256.0 / (256.0 - th)
    base = (((seed & m32) ^ ((seed >> 32) & m32)) + (slab * c3)) & m32
    q = torch.arange(nq, dtype=torch.int64, device=device)[:, None]
    k = torch.arange(nk, dtype=torch.int64, device=device)[None, :]
    u = (base + (q >> 1) * c1 + (k >> 1) * c2) & m32
    u = u ^ (u >> 16)
    u = (u * 0x7FEB352D) & m32
    u = u ^ (u >> 15)
    field = (u >> (16 * (q & 1) + 8 * (k & 1))) & 0xFF
    return (field >= th).to(torch.float64) * ks


def _mul32(a, c):
    """(a * c) mod 2^32 for int64 tensors a < 2^32 and a 32-bit constant c, in 16-bit halves (no int64 overflow)."""
    return ((a & 0xFFFF) * c + ((((a >> 16) * c) & 0xFFFF) << 16)) & 0xFFFFFFFF


def elem_dropout_scale(seed: int, idx, p: float):
    """The element-wise dropout mask of the GraphNorm, LayerNorm and bias+GELU kernels (``hash_u32`` / ``dropout_scale`` /
    ``dropout_keep_bits``, common.hpp), restated with torch integer arithmetic (checker only; DESIGN.md section 4 'Dropout').
    ``idx``: int64 tensor of element offsets in the row-major tensor (r * f + c).  One 32-bit word decides the pair idx >> 1:
    w = lowbias32(lo32(i) * C1 + hi32(i) * C2 + lo32(seed)) ^ hi32(seed) with i = idx >> 1; the element's field is the 16-bit
    half (idx & 1) of w, kept when field >= th = lround(p * 65536) clamped to 65535.  Returns a float32 tensor of idx's shape:
    0 or the fp32 keep scale 65536f / (65536f - th)."""
    m32 = 0xFFFFFFFF
    th = 0 if p <= 0 else int(np.floor(np.float32(p) * np.float32(65536.0) + np.float32(0.5)))
    th = max(0, min(65535, th))
    ks = np.float32(65536.0) / (np.float32(65536.0) - np.float32(th))
    idx = torch.as_tensor(idx, dtype=torch.int64)
    i = idx >> 1
    x = (_mul32(i & m32, 0x9E3779B1) + _mul32(i >> 32, 0x85EBCA77) + (seed & m32)) & m32
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    x = x ^ (x >> 16)
    x = x ^ ((seed >> 32) & m32)
    field = (x >> (16 * (idx & 1))) & 0xFFFF
    return (field >= th).to(torch.float32) * float(ks)


def _dense_reference(q, k, v, go, h, scale, kv_len=None, drop=None):
    """Dense softmax attention in float64, forward and autograd backward: q, go [b, lq, h*d], k, v [b, lk, h*d] (any float
    dtype, any device) -> out, dq, dk, dv as float64 tensors of the same shapes.  Keys at or past ``kv_len[bi]`` (clamped to
    [0, lk], as the kernels do) take no part; a sequence with no valid key has zero output and zero gradients (the kernels'
    contract, gmlm_hip.h).  ``drop(bi, hi)`` -> [lq, lk] multiplier of the probabilities (0 or the keep scale).  Heads are
    batched, a few at a time so that one [heads, lq, lk] float64 tensor stays below 1 GiB."""
    b, lq, hd = q.shape
    lk, d = k.shape[1], hd // h
    outs = [torch.zeros(b, t_.shape[1], hd, dtype=torch.float64, device=q.device) for t_ in (q, q, k, v)]
    chunk = max(1, (1 << 27) // max(1, lq * lk))
    for bi in range(b):
        n = lk if kv_len is None else max(0, min(lk, int(kv_len[bi])))
        if n == 0:
            continue                                              # no valid key: zero output, zero gradients
        for h0 in range(0, h, chunk):
            h1 = min(h, h0 + chunk)
            heads = lambda t_, rows: t_[bi, :rows].detach().reshape(rows, h, d)[:, h0:h1].transpose(0, 1).double().contiguous()
            qq, kk, vv = (heads(t_, rows).requires_grad_(True) for t_, rows in ((q, lq), (k, n), (v, n)))
            p = torch.softmax((qq @ kk.transpose(1, 2)) * scale, -1)
            if drop is not None:
                p = p * torch.stack([drop(bi, hi)[:, :n] for hi in range(h0, h1)]).to(p)
            o = p @ vv
            o.backward(heads(go, lq))
            cols = slice(h0 * d, h1 * d)
            back = lambda t_: t_.transpose(0, 1).reshape(t_.shape[1], -1)
            outs[0][bi, :, cols], outs[1][bi, :, cols] = back(o.detach()), back(qq.grad)
            outs[2][bi, :n, cols], outs[3][bi, :n, cols] = back(kk.grad), back(vv.grad)
            del p, o
    return outs


def _close(name, got, ref, max_rel, l2_rel):
    """max |got - ref| / max |ref| <= max_rel and ||got - ref|| / ||ref|| <= l2_rel over the whole tensor."""
    got = got.double()
    e = got - ref
    mx, l2 = float(e.abs().max()) / float(ref.abs().max()), float(e.norm()) / float(ref.norm())
    print(f"  {name}: max|err| / max|ref| = {mx:.2e}, l2 rel = {l2:.2e}")
    assert mx <= max_rel and l2 <= l2_rel, (name, mx, l2)


def _bare_kernel_name(name):
    """'void gmlm::attn_fwd_kernel<float, 64, 2, false>(gmlm::AttnParams)' (or its mangled form) ->
    'attn_fwd_kernel<float, 64, 2, false>': no return type, no parameter list, no leading 'gmlm::'."""
    if name.startswith("_Z"):
        name = torch._C._demangle(name)
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, c in enumerate(name):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            name = name[:i]
            break
    return name[len("gmlm::"):] if name.startswith("gmlm::") else name


def kernels_run(fn):
    """Runs ``fn`` under the torch profiler and returns the set of the project's device kernels it launched, as bare template
    ids ('attn_bwd_dkv_kernel<unsigned short, 64, 4, true, 128>'; bf16 shows up as 'unsigned short').  Fails when the
    profiler saw no device kernel at all, so that a profiler that records nothing cannot make a name assertion pass."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    assert names, "the profiler recorded no device kernel"
    return {_bare_kernel_name(n) for n in names if "gmlm::" in n or n.startswith("_ZN4gmlm")}

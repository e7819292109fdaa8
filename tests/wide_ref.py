"""float64 numpy restatement of the input side of one layer, written from oracle/biogpt_oracle.c bo_eval: what the kernels of that layer are fed.

layer_stats(W, tokens, layer) walks the layers before `layer` in full (their output is this layer's input) and returns, for `layer`, the hidden state
that enters it, both LayerNorm outputs, the attention probabilities and the fc1 pre-activation.  `layer` == n_layer gives the final LayerNorm only.
W is {tensor name: float array}, the f32 tensors of a model file (wide_models.load_arrays).  Test infrastructure: conditions on the test's INPUT are
computed here, nothing here is a reference for a kernel's output."""
import math

import numpy as np

NORM_EPS = 1e-5          # biogpt_oracle.c NORM_EPS
_erf = np.frompyfunc(math.erf, 1, 1)


def _ln(x, g, b, eps):
    v = x - x.mean(axis=1, keepdims=True)
    return v / np.sqrt((v * v).mean(axis=1, keepdims=True) + eps) * g + b


def _gelu(x, hf):
    if hf:
        return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)).astype(np.float64))
    return 0.5 * x * (1.0 + np.tanh(0.79788456080286535588 * x * (1.0 + 0.044715 * x * x)))


def layer_stats(W, tokens, layer, n_batch=None, hf=False, n_head=16):
    """n_batch None: query i sees keys 0 .. i (single-token decode, and the oracle's causal mode).  n_batch = b: it sees every key of its own chunk of b
    tokens too (the reference has no mask inside an eval).  hf: erf GELU and eps 1e-12, the arithmetic of OracleModel(mode="hf")."""
    f = lambda name: np.asarray(W[name], dtype=np.float64)
    n_layer = 1 + max(int(k.split(".")[2]) for k in W if k.startswith("biogpt.layers."))
    toks = np.asarray(tokens)
    n = toks.size
    Dm = W["biogpt.embed_tokens.weight"].shape[1]
    eps = 1e-12 if hf else NORM_EPS
    x = f("biogpt.embed_tokens.weight")[toks] * math.sqrt(Dm) + f("biogpt.embed_positions.weight")[np.arange(n) + 2]
    last = np.arange(n) if n_batch is None else np.minimum((np.arange(n) // n_batch + 1) * n_batch, n) - 1
    visible = np.arange(n)[None, :] <= last[:, None]                     # [query, key]
    taps = [x]
    for l in range(n_layer + 1):
        if l == n_layer:
            out = dict(x_in=x, ln0=_ln(x, f("biogpt.layer_norm.weight"), f("biogpt.layer_norm.bias"), eps))
            break
        p = "biogpt.layers.%d." % l
        h0 = _ln(x, f(p + "self_attn_layer_norm.weight"), f(p + "self_attn_layer_norm.bias"), eps)
        dk = Dm // n_head
        q = (h0 @ f(p + "self_attn.q_proj.weight").T + f(p + "self_attn.q_proj.bias")) / math.sqrt(dk)
        k = h0 @ f(p + "self_attn.k_proj.weight").T + f(p + "self_attn.k_proj.bias")
        v = h0 @ f(p + "self_attn.v_proj.weight").T + f(p + "self_attn.v_proj.bias")
        qh, kh, vh = (a.reshape(n, n_head, dk).transpose(1, 0, 2) for a in (q, k, v))
        s = qh @ kh.transpose(0, 2, 1)                                   # [head, query, key]
        s = np.where(visible[None], s, -np.inf)
        s_rel = s - s.max(axis=2, keepdims=True)
        e = np.exp(s_rel)
        probs = e / e.sum(axis=2, keepdims=True)
        att = (probs @ vh).transpose(1, 0, 2).reshape(n, Dm)
        inp_ff = att @ f(p + "self_attn.out_proj.weight").T + f(p + "self_attn.out_proj.bias") + x
        h1 = _ln(inp_ff, f(p + "final_layer_norm.weight"), f(p + "final_layer_norm.bias"), eps)
        pre = h1 @ f(p + "fc1.weight").T + f(p + "fc1.bias")
        if l == layer:
            out = dict(x_in=x, ln0=h0, ln1=h1, scores=s, probs=probs, visible=visible, pre_gelu=pre)
            break
        x = _gelu(pre, hf) @ f(p + "fc2.weight").T + f(p + "fc2.bias") + inp_ff
        taps.append(x)
    out["taps"] = taps                # taps[k]: hidden state after layer k - 1 (taps[0]: embeddings) = OracleModel.tap(k - 1)
    return out


def q8_blocks(rows):
    """The scalar Q8_0 / Q8_1 activation quantizer (quantize_row_q8_0) on float32 rows [n, K]: (amax [n, K/32] float32, codes [n, K/32, 32] int)."""
    x = np.asarray(rows, dtype=np.float32).reshape(rows.shape[0], -1, 32)
    amax = np.abs(x).max(axis=2)
    d = (amax / np.float32(127.0)).astype(np.float32)
    inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    v = (x * inv[:, :, None]).astype(np.float32)
    codes = (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int32)      # roundf: half away from zero
    return amax, codes


def f16_patterns(x):
    """Distinct f16 bit patterns among float values (the index into the fp16 GELU table)."""
    return np.unique(np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16))

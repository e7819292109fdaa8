"""Full-width model files off the operating point of write_synthetic (every matrix and bias N(0, 0.02), every LayerNorm gain 1 +- 0.02).

A write_synthetic f32 file at the widths of test_gpu_fullsize.KW is read with modelfile_py, transformed with numpy and written back; the
quantized files come from the package's own quantize_file.  Each transformation ("ingredient") is its own function, build() applies one of
them or all ("combined").  tests/test_wide_models.py proves on the CPU that the files are what they claim (wide_ref.layer_stats), and
compared_rows() and the plan functions state once which oracle rows tests/test_gpu_wide.py compares, so that the CPU test can look at exactly those rows.

Starting factors are the issue's estimates; where a condition of test_wide_models.py needed another value the reason stands beside it."""
import numpy as np

from modelfile_py import read_model, write_model
from test_gpu_fullsize import KW

SEED = 0x57494445
QUANT = ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]
INGREDIENTS = ["peaked", "gelu", "outlier", "dead"]
L, D, F, V, P = KW["n_layer"], KW["d_model"], KW["d_ff"], KW["n_vocab"], KW["n_positions"]

# outlier: where the special channels of a LayerNorm live (the same in every LayerNorm that gets them)
OUT_HOT = (77, 613)            # gain x HOT_GAIN: each dominates its 32-channel activation block
OUT_ZERO_BLOCK = 5             # channels 160 .. 191: gain 0, bias 0   -> a Q8 block with amax == 0
OUT_CONST_BLOCK = 21           # channels 672 .. 703: gain 0, bias 0.3 -> a Q8 block of 32 equal values
OUT_BIAS_CH, OUT_BIAS = 300, 50.0
HOT_GAIN = 200.0
# A hot channel at x 200 alone leaves its 31 block neighbours at Q8 code 0 only when its |z| exceeds 254 / 200 times the largest neighbour (about 2.5 for
# 31 values of N(0, 1)): a 3.2-sigma event, not met on a few hundred rows.  The neighbours of the second hot channel therefore get gain x 0.05.
NEIGHBOUR_GAIN = 0.05
# dead: the values of the 8 constant rows, all different (two equal rows of output_projection would be two equal logits)
CONST_ROWS = [-0.03, -0.02, -0.011, -0.004, 0.004, 0.011, 0.02, 0.03]


def lname(l, what):
    return "biogpt.layers.%d.%s" % (l, what)


def load_arrays(path):
    """(hp, vocab, merges, names in file order, {name: float32 array [ne1, ne0] or [ne0]}) of an all-f32 file; the arrays are read-only views."""
    hp, vocab, merges, tensors = read_model(path)
    W, order = {}, []
    for t in tensors:
        assert t["type"] == 0, t["name"]
        a = np.frombuffer(t["raw"], dtype=np.float32)
        W[t["name"]] = a.reshape(t["ne"][1], t["ne"][0]) if len(t["ne"]) == 2 else a
        order.append(t["name"])
    return hp, vocab, merges, order, W


def save_arrays(path, hp, vocab, merges, order, W, f16=False):
    tensors = []
    for name in order:
        a = W[name]
        ne = [a.shape[1], a.shape[0]] if a.ndim == 2 else [a.shape[0]]
        if f16 and a.ndim == 2 and name.endswith(".weight"):      # convert.py --use-f16: the 2-D "*.weight" tensors as float16, ftype 1
            tensors.append(dict(name=name, type=1, ne=ne, raw=a.astype(np.float16).tobytes()))
        else:
            tensors.append(dict(name=name, type=0, ne=ne, raw=np.ascontiguousarray(a, dtype=np.float32).tobytes()))
    write_model(path, dict(hp, ftype=int(f16)), vocab, merges, tensors)


def _own(W, name):
    if not W[name].flags.writeable:
        W[name] = W[name].copy()
    return W[name]


def peaked(W):
    """q_proj / k_proj weight and bias x 4 (layer 0) and x 12 (layer 1): scores x 16 and x 144.  Layer 2 is the control."""
    for l, f in ((0, 4.0), (1, 12.0)):
        for proj in ("q_proj", "k_proj"):
            for part in ("weight", "bias"):
                _own(W, lname(l, "self_attn.%s.%s" % (proj, part)))[...] *= np.float32(f)


def gelu(W):
    """fc1 weight x 8 in layers 0 and 1, fc1 bias a shuffled ramp -8.5 .. +8.5: pre-GELU values over the table's whole useful range, |x| < 100, far
    below f16's 65,504.  (A ramp of -12 .. +12, the issue's start, leaves 2 / 24 = 8.3 % of the values in [-1, 1] whatever the weights; 2 / 17 = 11.8 %.)"""
    rng = np.random.default_rng(SEED + 1)
    for l in (0, 1):
        _own(W, lname(l, "fc1.weight"))[...] *= np.float32(8.0)
        _own(W, lname(l, "fc1.bias"))[...] = rng.permutation(np.linspace(-8.5, 8.5, F)).astype(np.float32)


def outlier(W):
    """First LayerNorm of every layer and the final one: two hot channels (the second with quiet neighbours), one block that is exactly 0, one block
    that is exactly 0.3.
    Second LayerNorm of layer 1: one channel with bias 50.  Layer 0's q / k columns of the hot channels and layer 1's fc1 column of the bias channel
    are scaled back (below)."""
    for pre in [lname(l, "self_attn_layer_norm") for l in range(L)] + ["biogpt.layer_norm"]:
        g, b = _own(W, pre + ".weight"), _own(W, pre + ".bias")
        blk = OUT_HOT[1] // 32 * 32
        g[blk:blk + 32] *= np.float32(NEIGHBOUR_GAIN)
        g[OUT_HOT[1]] /= np.float32(NEIGHBOUR_GAIN)
        for ch in OUT_HOT:
            g[ch] *= np.float32(HOT_GAIN)
        for blk, c in ((OUT_ZERO_BLOCK, 0.0), (OUT_CONST_BLOCK, 0.3)):
            g[32 * blk:32 * blk + 32] = 0.0
            b[32 * blk:32 * blk + 32] = np.float32(c)
    _own(W, lname(1, "final_layer_norm.bias"))[OUT_BIAS_CH] = np.float32(OUT_BIAS)
    # The special channels are there for the activation quantizer and the LayerNorm kernels.  Where they would swamp another ingredient's condition in the
    # combined file their weight columns are scaled back: layer 0's q / k columns of the hot channels (scores x 100 otherwise: layer 0 one-hot, no mid-range
    # softmax left) and layer 1's fc1 column of the bias-50 channel (a term of deviation 8 on every pre-activation otherwise: 7 % left in [-1, 1]).
    for proj in ("q_proj", "k_proj"):
        _own(W, lname(0, "self_attn.%s.weight" % proj))[:, list(OUT_HOT)] *= np.float32(1.0 / HOT_GAIN)
    _own(W, lname(1, "fc1.weight"))[:, OUT_BIAS_CH] *= np.float32(1.0 / OUT_BIAS)


def dead_rows(n_rows, seed):
    """The 40 rows a matrix gives up, five kinds of 8, chosen by seed."""
    rows = np.random.default_rng(seed).choice(n_rows, 40, replace=False)
    return dict(zero=rows[0:8], const=rows[8:16], tiny=rows[16:24], subnormal=rows[24:32], spike=rows[32:40])


def dead(W):
    """q_proj, v_proj, fc1, fc2 (every layer) and output_projection: 256 scattered zero blocks, 8 zero rows, 8 constant rows (Q4_1 / Q5_1: d = 0, m = c),
    8 rows of N(0, 1e-7) (block scales round to 0 or to the smallest f16 subnormal while the codes are not 0), 8 rows of N(0, 2e-5) (scales are f16
    subnormals in every block type: the issue's 1e-7 gives amax / 127 = 2e-9 = 0 in Q8_0), 8 rows of N(0, 1e-3) with one +-1.0 per block."""
    names = [lname(l, "self_attn.%s.weight" % p) for l in range(L) for p in ("q_proj", "v_proj")]
    names += [lname(l, "%s.weight" % p) for l in range(L) for p in ("fc1", "fc2")] + ["output_projection.weight"]
    for k, name in enumerate(names):
        m = _own(W, name)
        rng = np.random.default_rng(SEED + 100 + k)
        R, K = m.shape
        for r, b in zip(rng.integers(0, R, 256), rng.integers(0, K // 32, 256)):
            m[r, 32 * b:32 * b + 32] = 0.0
        kinds = dead_rows(R, SEED + 200 + k)
        m[kinds["zero"]] = 0.0
        m[kinds["const"]] = rng.permutation(CONST_ROWS).astype(np.float32)[:, None]
        m[kinds["tiny"]] = (1e-7 * rng.standard_normal((8, K))).astype(np.float32)
        m[kinds["subnormal"]] = (2e-5 * rng.standard_normal((8, K))).astype(np.float32)
        spike = (1e-3 * rng.standard_normal((8, K))).astype(np.float32)
        at = rng.integers(0, 32, (8, K // 32)) + 32 * np.arange(K // 32)
        np.put_along_axis(spike, at, rng.choice([-1.0, 1.0], at.shape).astype(np.float32), axis=1)
        m[kinds["spike"]] = spike


APPLY = dict(peaked=peaked, gelu=gelu, outlier=outlier, dead=dead)


def transformed(W, which):
    """A copy-on-write transformed view of the arrays: which = an ingredient, "combined" or "plain"."""
    out = dict(W)
    for name in (INGREDIENTS if which == "combined" else [] if which == "plain" else [which]):
        APPLY[name](out)
    return out


def raw_q8_edit(src, dst):
    """A Q8_0 file edited after quantization: in q_proj and fc2 of every layer 64 blocks get all codes -128, 64 all +127, 64 a negated scale.
    The format allows all three; no quantizer emits them."""
    hp, vocab, merges, tensors = read_model(src)
    rng = np.random.default_rng(SEED + 300)
    for t in tensors:
        if t["type"] == 8 and (".q_proj.weight" in t["name"] or ".fc2.weight" in t["name"]):
            blk = np.frombuffer(t["raw"], dtype=np.uint8).reshape(-1, 34).copy()
            pick = rng.choice(blk.shape[0], 192, replace=False)
            blk[pick[:64], 2:] = 0x80
            blk[pick[64:128], 2:] = 0x7F
            blk[pick[128:], 1] ^= 0x80          # sign bit of the f16 scale
            t["raw"] = blk.tobytes()
    write_model(dst, hp, vocab, merges, tensors)


def build(pkg, d, want):
    """Write the files named in `want` ("<which>.<type>", which in INGREDIENTS + combined / plain, type in QUANT + f32 / f16, or "rawq8") into directory d.
    Returns {name: path}.  The f32 files that were only needed as quantizer input are removed."""
    import os
    base = os.path.join(str(d), "plain.f32.bin")
    pkg.write_synthetic(base, **KW)
    hp, vocab, merges, order, W = load_arrays(base)
    out, need = {}, {}
    for name in want:
        which, typ = ("combined", "rawq8") if name == "rawq8" else name.split(".")
        need.setdefault(which, []).append(typ)
    for which, types in need.items():
        f32 = base if which == "plain" else os.path.join(str(d), which + ".f32.bin")
        if which != "plain":
            T = transformed(W, which)
            save_arrays(f32, hp, vocab, merges, order, T)
            if "f16" in types:
                out[which + ".f16"] = os.path.join(str(d), which + ".f16.bin")
                save_arrays(out[which + ".f16"], hp, vocab, merges, order, T, f16=True)
            del T
        for typ in types:
            if typ in QUANT or typ == "rawq8":
                q = "q8_0" if typ == "rawq8" else typ
                path = os.path.join(str(d), "%s.%s.bin" % (which, q))
                if not os.path.exists(path):
                    pkg.quantize_file(f32, path, q)
                if typ == "rawq8":
                    out["rawq8"] = os.path.join(str(d), "rawq8.bin")
                    raw_q8_edit(path, out["rawq8"])
                    if "q8_0" not in types:
                        os.remove(path)
                else:
                    out[which + "." + typ] = path
        if "f32" in types:
            out[which + ".f32"] = f32
        elif which != "plain":
            os.remove(f32)
    if "plain.f32" not in out:
        os.remove(base)
    return out


# ---- which oracle rows the GPU test compares: stated once, walked by the GPU test and by the CPU test ----

FILES = ["combined." + t for t in QUANT + ["f32", "f16"]] + ["rawq8"] + [w + ".q4_0" for w in INGREDIENTS]
BLOCK_FILES = [n for n in FILES if not n.endswith((".f32", ".f16"))]
FLOAT_FILES = ["combined.f32", "combined.f16"]

# Prompt seeds per (file, scenario), default 1: searched on the CPU so that every compared row has an oracle top-two gap >= 2e-3 (test_wide_models.py
# asserts it for every row; nothing is skipped).  About 2 % of the rows of a file with an ordinary final LayerNorm fall below that gap.
SEED_TABLE = {("combined.q4_1", "decode"): 2, ("combined.q5_1", "chunks"): 3, ("rawq8", "chunks"): 2, ("gelu.q4_0", "decode"): 6, ("dead.q4_0", "decode"): 3}


def seed_of(name, scenario):
    return SEED_TABLE.get((name, scenario), 1)


def tokens(seed, n):
    rng = np.random.default_rng(seed)
    return [2] + [int(v) for v in rng.integers(4, V, n - 1)]


def top_two_gap(row):
    a = np.partition(row, -2)[-2:]
    return float(a[1] - a[0])


def decode_rows(o, seed, n_steps=71):
    """Item 1: teacher-forced single-token decode from 0 keys on (first token by seed); yields (token, n_past, oracle row)."""
    tok = int(np.random.default_rng(seed).integers(4, V))
    for n_past in range(n_steps):
        lo = o.eval([tok], n_past)
        yield tok, n_past, lo
        tok = int(lo.argmax())


def chunk_plan(seed):
    """Items 2 and 4 on one context: [(tokens, n_past, compared)]: chunks of 8 over 0 .. 40 keys, an uncompared fill to 248, chunks of 8 over 248 .. 304
    (the column-per-XCD launch on both sides of 256 keys), one eval of 19 tokens (the 8-column chain), then 4 single tokens beyond 300 keys."""
    t = tokens(seed, 327)
    plan = [(t[a:a + 8], a, True) for a in range(0, 40, 8)]
    plan += [(t[a:a + 8], a, False) for a in range(40, 248, 8)]
    plan += [(t[a:a + 8], a, True) for a in range(248, 304, 8)]
    plan += [(t[304:323], 304, True)]
    plan += [(t[a:a + 1], a, True) for a in range(323, 327)]
    return plan


def prompt_row(o, toks, n_batch=8):
    """The oracle fed a prompt the way the reference's loop feeds it: chunks of n_batch; returns the last chunk's row."""
    lo = None
    for at in range(0, len(toks), n_batch):
        lo = o.eval(toks[at:at + n_batch], at)
    return lo


def float_plan(seed):
    """Item 5: [(tokens, n_past, compared)] for float files: an 8-token chunk, single tokens below 224 keys, a fill, single tokens at 230 keys."""
    t = tokens(seed, 233)
    plan = [(t[0:8], 0, True)] + [(t[a:a + 1], a, True) for a in range(8, 12)]
    plan += [(t[a:a + 8], a, False) for a in range(12, 220, 8)]
    plan += [(t[a:a + 1], a, True) for a in (220, 221)] + [(t[222:230], 222, False)] + [(t[a:a + 1], a, True) for a in (230, 231, 232)]
    return plan


def long_plan(seed):
    """Item 4 with the key-range helpers of kernels_xlong.hip.h (the GPU test loads with BIOGPT_HIP_XPIPE_DUAL=0; by default contexts of 257 .. 512 keys take
    two workgroups per head of the short-context kernel instead): [(tokens, n_past, compared)]: 300 tokens in chunks of 8, then 4 single tokens."""
    t = tokens(seed, 304)
    return [(t[a:min(a + 8, 300)], a, False) for a in range(0, 300, 8)] + [(t[a:a + 1], a, True) for a in range(300, 304)]


def compared_rows(O, name, path, n_threads=8):
    """Every oracle row on which the GPU test compares an arg-max for file `name`: yields (scenario, n_past, row)."""
    if name in BLOCK_FILES:
        o = O.OracleModel(path, n_threads=n_threads)
        for tok, n_past, lo in decode_rows(o, seed_of(name, "decode")):
            yield "decode", n_past, lo
        o = O.OracleModel(path, n_threads=n_threads)
        yield "prompt", 96, prompt_row(o, tokens(seed_of(name, "prompt"), 96))
        if name == "combined.q4_0":
            o = O.OracleModel(path, n_threads=n_threads)
            yield "prompt700", 700, prompt_row(o, tokens(seed_of(name, "prompt700"), 700))
    plan = None
    if name in BLOCK_FILES and (name.startswith("combined.") or name == "rawq8"):
        plan, what = chunk_plan(seed_of(name, "chunks")), "chunks"
    if name in FLOAT_FILES:
        plan, what = float_plan(seed_of(name, "floats")), "floats"
    plans = [(what, plan)] if plan else []
    if plan and what == "chunks":
        plans.append(("long", long_plan(seed_of(name, "long"))))
    for what, plan in plans:
        o = O.OracleModel(path, n_threads=n_threads)
        for toks, n_past, compared in plan:
            lo = o.eval(toks, n_past)
            if compared:
                yield what, n_past, lo


# ---- tied files (tests/test_tail_files.py, tests/test_gpu_tail_calls.py): an lm_head made of copies of a few base rows, so every logit value recurs --------------
# Classes of rows: four "early" ones share rows 0 .. 63 (a tie inside the first partial block), n_cyc "cyclic" ones take turns from row 64 to row V - 17 (copies in
# every later 64-row block and every 256-row workgroup: the winner's lowest copy lies in the SECOND partial), four "last" ones share rows V - 16 .. V - 1, the
# 16-row block of the last partial.  Layout "a" has 32 cyclic classes of 1322 copies (topk_kernel answers), layout "b" 8 of 5288 -- more than topk_kernel's 4096
# candidate slots whenever one of them wins.  The early and last base rows are longer, so that they win their share of the steps.
TIED_SEED = {"a": 1, "b": 1}
TIED_CYC = {"a": 32, "b": 8}
TIED_EARLY_GAIN, TIED_LAST_GAIN = 1.3, 1.6
TIED_K = 40
TAIL_TYPES = QUANT + ["f32"]


def tied_classes(layout):
    n_cyc = TIED_CYC[layout]
    r = np.arange(V)
    c = 4 + (r - 64) % n_cyc
    c[:64] = r[:64] % 4
    c[V - 16:] = 4 + n_cyc + r[V - 16:] % 4
    return c


def tied(W, layout):
    n = 4 + TIED_CYC[layout] + 4
    base = (0.02 * np.random.default_rng(SEED + 400).standard_normal((n, D))).astype(np.float32)
    base[:4] *= np.float32(TIED_EARLY_GAIN)
    base[-4:] *= np.float32(TIED_LAST_GAIN)
    W["output_projection.weight"] = base[tied_classes(layout)]


# tail_q8: lm_head rows of the Q8_0 tied file whose first block gets another scale.  An f16 NaN gives a NaN logit at every step; +-inf gives +inf, -inf (by the
# sign of the block's dot) or NaN (a dot of 0).  NaNs stand in the FIRST finisher lane of blocks 1 and 2 (rows 64, 128: the lowest copies of every cyclic class lie
# behind them in block 1), in a middle lane of the in-launch kernels' and lm_stream_kernel's groups (row 64 * 3 + 34, the block's next rows behind it) and in the last
# row; two rows of ONE class (equal codes: equal logits, tied at +-inf) carry +inf, the lower one behind the NaN of block 2; a row of the last block carries -inf.
TAIL_NAN_ROWS = (64, 128, 64 * 3 + 34, V - 1)
TAIL_PINF_ROWS = (128 + 2, 128 + 2 + 32 * 40)        # (r - 64) % 32 equal: one class in layout "a"
TAIL_NINF_ROWS = (V - 14,)


def tail_q8_edit(src, dst):
    hp, vocab, merges, tensors = read_model(src)
    for t in tensors:
        if t["name"] == "output_projection.weight":
            assert t["type"] == 8
            blk = np.frombuffer(t["raw"], dtype=np.uint8).reshape(V, D // 32, 34).copy()
            for rows, bits in ((TAIL_NAN_ROWS, 0x7E00), (TAIL_PINF_ROWS, 0x7C00), (TAIL_NINF_ROWS, 0xFC00)):
                blk[list(rows), 0, 0:2] = np.array([bits], "<u2").view(np.uint8)
            t["raw"] = blk.tobytes()
    write_model(dst, hp, vocab, merges, tensors)


def build_tail(pkg, d, want):
    """Write the tied files named in `want` ("tied_a.<type>", "tied_b.<type>", type in TAIL_TYPES, or "tail_q8") into directory d; returns {name: path}."""
    import os
    base = os.path.join(str(d), "plain.f32.bin")
    pkg.write_synthetic(base, **KW)
    hp, vocab, merges, order, W = load_arrays(base)
    out = {}
    for layout in ("a", "b"):
        types = [n.split(".")[1] for n in want if n.startswith("tied_%s." % layout)] + (["q8_0"] if layout == "a" and "tail_q8" in want else [])
        if not types:
            continue
        T = dict(W)
        tied(T, layout)
        f32 = os.path.join(str(d), "tied_%s.f32.bin" % layout)
        save_arrays(f32, hp, vocab, merges, order, T)
        del T
        for typ in dict.fromkeys(types):
            if typ == "f32":
                continue
            path = os.path.join(str(d), "tied_%s.%s.bin" % (layout, typ))
            pkg.quantize_file(f32, path, typ)
            if "tied_%s.%s" % (layout, typ) in want:
                out["tied_%s.%s" % (layout, typ)] = path
            if layout == "a" and typ == "q8_0" and "tail_q8" in want:
                out["tail_q8"] = os.path.join(str(d), "tail_q8.bin")
                tail_q8_edit(path, out["tail_q8"])
        if "tied_%s.f32" % layout in want:
            out["tied_%s.f32" % layout] = f32
        else:
            os.remove(f32)
    os.remove(base)
    return out


TAIL_FILES = ["tied_a." + t for t in TAIL_TYPES] + ["tied_b.q4_0", "tail_q8"]
TAIL_STEPS, TAIL_LONG, TAIL_LONG_STEPS = 6, 264, 4


def tail_prompt(name, which=0):
    """The 8-token prompt of a file's short calls (which 0, 1: the two columns of the batched call); the 264-token one of the calls past 256 keys (which 2)."""
    seed = 7000 + 10 * sorted(TAIL_FILES).index(name) + which
    return tokens(seed, TAIL_LONG if which == 2 else 8)


def tail_rows(o, prompt, n_steps):
    """Greedy decoding by the tail's rule on the oracle's rows: yields (n_past of the row's last token + 1, oracle row, id by tail_ref.argmax), the id fed back."""
    import tail_ref
    lo = prompt_row(o, prompt)
    n_past = len(prompt)
    for _ in range(n_steps):
        tok = tail_ref.argmax(lo)
        yield n_past, lo, tok
        lo = o.eval([tok], n_past)
        n_past += 1


def tail_plan(name):
    """[(what, prompt, steps)]: the greedy sequences the GPU test compares on file `name`; every row of them is also a row of its top-k comparisons."""
    plan = [("short", tail_prompt(name, 0), TAIL_STEPS)]
    if name in ("tied_a.q4_0", "tail_q8"):
        plan += [("second column", tail_prompt(name, 1), TAIL_STEPS), ("long", tail_prompt(name, 2), TAIL_LONG_STEPS)]
    return plan

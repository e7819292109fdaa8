"""Converter counterpart: HF checkpoint directory -> ggml-model.bin."""
import json
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def hf_dir(tmp_path_factory):
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    d = tmp_path_factory.mktemp("hf")
    cfg = tr.BioGptConfig(vocab_size=96, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                          intermediate_size=128, max_position_embeddings=32)
    torch.manual_seed(3)
    model = tr.BioGptForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 1:
                p.add_(0.05 * torch.randn_like(p))
    torch.save(model.state_dict(), d / "pytorch_model.bin")
    json.dump(dict(vocab_size=96, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=32,
                   intermediate_size=128, hidden_size=64), open(d / "config.json", "w"))
    json.dump({("w%d</w>" % i): i for i in range(96)}, open(d / "vocab.json", "w"))
    (d / "merges.txt").write_text("#version: 0.2\n" + "\n".join("x%d y%d 7" % (i, i) for i in range(9)) + "\n")
    return str(d), model


def test_converted_file_matches_hf_logits(pkg, oracle, hf_dir, tmp_path):
    import torch
    from biogpt_cpp_amd import convert_hf
    d, model = hf_dir
    out = convert_hf.convert(d, str(tmp_path / "m.bin"))
    o = oracle.OracleModel(out, mode="hf")
    assert (o.n_vocab, o.n_layer, o.n_head, o.n_positions, o.d_ff, o.d_model, o.ftype, o.n_merges) == (96, 2, 4, 32, 128, 64, 0, 10)
    toks = [2, 5, 17, 90, 33, 8]
    with torch.no_grad():
        ref = model(input_ids=torch.tensor([toks])).logits[0].numpy()
    got = o.eval(toks, 0, all_rows=True)
    # default HF init (std 0.02) makes the pre-LayerNorm variance tiny, which amplifies f32-vs-double round-off
    assert np.abs(got - ref).max() < 5e-4 and (got.argmax(1) == ref.argmax(1)).all()
    f16 = convert_hf.convert(d, str(tmp_path / "h.bin"), use_f16=True)
    assert oracle.OracleModel(f16).ftype == 1


@pytest.fixture(scope="module")
def golden_hf_dir(tmp_path_factory, golden_dir):
    """The HF checkpoint directory that tests/golden/make_golden.py gave the reference's converter (convert.py parse_hparams /
    parse_vocab / parse_bpe_merges / parse_model), rebuilt from what that converter wrote into tiny_f32.bin: the header, the vocab
    in id order, the merge lines, and every tensor's name, shape and float32 data in state-dict order."""
    torch = pytest.importorskip("torch")
    import modelfile_py
    hp, vocab, merges, tensors = modelfile_py.read_model(os.path.join(golden_dir, "tiny_f32.bin"))
    d = tmp_path_factory.mktemp("hf_golden")
    json.dump(dict(vocab_size=hp["n_vocab"], num_hidden_layers=hp["n_layer"], num_attention_heads=hp["n_head"], max_position_embeddings=hp["n_positions"],
                   intermediate_size=hp["d_ff"], hidden_size=hp["d_model"]), open(d / "config.json", "w"))
    json.dump({t.decode("utf-8"): i for i, t in enumerate(vocab)}, open(d / "vocab.json", "w"))
    # make_golden.py's merge lines carry a third field ("a0 b0 1"); the file keeps the first two, as convert.py does
    (d / "merges.txt").write_text("".join(m.decode("utf-8") + ("\n" if m.startswith(b"#") else " 1\n") for m in merges), encoding="utf-8")
    sd = {}
    for t in tensors:
        assert t["type"] == 0
        sd[t["name"]] = torch.from_numpy(np.frombuffer(t["raw"], dtype=np.float32).reshape(t["ne"][::-1]).copy())
    torch.save(sd, d / "pytorch_model.bin")
    return str(d)


@pytest.mark.parametrize("f16", [False, True])
def test_bytes_identical_to_reference_converter(pkg, golden_hf_dir, golden_dir, tmp_path, f16):
    """Our converter on the checkpoint the reference's convert.py was given writes the bytes that convert.py wrote (tiny_f32.bin /
    tiny_f16.bin, committed outputs of the reference's own writer functions)."""
    from biogpt_cpp_amd import convert_hf
    mine = convert_hf.convert(golden_hf_dir, str(tmp_path / "mine.bin"), use_f16=f16)
    ref = os.path.join(golden_dir, "tiny_f16.bin" if f16 else "tiny_f32.bin")
    assert open(mine, "rb").read() == open(ref, "rb").read()

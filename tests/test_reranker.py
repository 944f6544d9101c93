"""CrossEncoderReranker mirror (reference src/rag/reranker.py:26-216) on the CPU: the golden fixture of the reference's own rerank and
document rebuild (tests/golden/reranker_golden.json), the interface, the packed pair forward against transformers' module forward,
local checkpoints and the librdx entry points' argument checks."""
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from rag_dpo_amd import reranker as RR
from rag_dpo_amd.retriever import RetrievedChunk, documents_from_ranked_chunks

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import reranker_world as W  # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "reranker_golden.json"), encoding="utf-8"))


class FakeModel:
    """a model object with only sentence-transformers' predict(): records what it is handed, returns scripted float32 scores"""

    def __init__(self, scores, raises=False):
        self.scores, self.raises, self.calls = scores, raises, []

    def predict(self, pairs, batch_size=32, show_progress_bar=True):
        self.calls.append({"pairs": [list(p) for p in pairs], "batch_size": batch_size, "show_progress_bar": show_progress_bar})
        if self.raises:
            raise RuntimeError("scripted model failure")
        return np.asarray(self.scores, dtype=np.float32)


class ScriptedMatcher:
    """replays the boosts the reference's TopicMatcher returned for each (topics, tags) call"""

    def __init__(self, calls):
        self.table = {(tuple(t), tags): float(b) for t, tags, b in calls}
        self.seen = []

    def topic_boost(self, question_topics, chunk_tags_str):
        self.seen.append([list(question_topics), chunk_tags_str])
        return self.table[(tuple(question_topics), chunk_tags_str)]


def case_chunks(case):
    pool = W.pool()
    return [RetrievedChunk(chunk_id=pool[i]["chunk_id"], text=pool[i]["text"], document_path=pool[i]["document_path"],
                           chunk_nature=pool[i]["metadata"]["chunk_nature"], chunk_index=pool[i]["metadata"]["chunk_index"],
                           confidence=pool[i]["metadata"].get("confidence", "unknown"), distance=pool[i]["distance"],
                           metadata=pool[i]["metadata"]) for i in case["idx"]]


def run_case(case, gold, device="cpu"):
    """-> (result, model, matcher) of rag_dpo_amd's rerank on one fixture case"""
    r = RR.CrossEncoderReranker(device=device, min_score=case["min_score"])
    r._model = FakeModel(case["scores"], raises=case["raises"])
    matcher = ScriptedMatcher(gold["boosts"]) if gold["boosts"] is not None else None
    out = r.rerank(W.QUERY, case_chunks(case), top_k=case["top_k"], topic_matcher=matcher, question_topics=case["topics"])
    return out, r._model, matcher


def check_against_gold(case, gold, out, model, matcher):
    assert model.calls == gold["model_calls"], case["name"]              # pairs (heading, character cut), batch size, no progress bar
    if matcher is not None:
        assert matcher.seen == [c[:2] for c in gold["boosts"]], case["name"]
    if "raises" in gold:                                                 # documented difference: the reference's log line raises
        assert gold["raises"] == "IndexError" and out == [], case["name"]
        return
    chunks = case_chunks(case)
    got = [{"chunk_id": r.chunk_id, "rerank_score": repr(float(r.rerank_score)), "original_rank": r.original_rank,
            "document_path": r.document_path, "text_is_input": r.text == chunks[r.original_rank].text} for r in out]
    assert got == gold["result"], case["name"]
    assert all(type(r.rerank_score) is float for r in out)
    docs = documents_from_ranked_chunks(out)
    assert [{"document_path": d.document_path, "avg_similarity": repr(float(d.avg_similarity)), "primary_nature": d.primary_nature,
             "chunks": [[c.chunk_id, repr(float(c.hybrid_score)), repr(float(c.distance)), c.chunk_nature, c.chunk_index, c.confidence]
                        for c in d.chunks]} for d in docs] == gold["documents"], case["name"]


def test_golden_fixture_reproduced_on_cpu():
    cases = W.cases()
    assert [c["name"] for c in cases] == [g["name"] for g in GOLDEN["cases"]]
    assert GOLDEN["query"] == W.QUERY
    for case, gold in zip(cases, GOLDEN["cases"]):
        check_against_gold(case, gold, *run_case(case, gold))
    names = {g["name"] for g in GOLDEN["cases"]}
    assert {"exact_ties", "straddling_min_score", "keep3_top_k_1", "keep3_top_k_2", "keep3_top_k_3", "top_k_beyond_n", "n_0", "n_1",
            "n_2", "headings_and_long_text", "boosts_reorder", "model_raises"} <= names


def test_fixture_covers_what_it_claims():
    by = {g["name"]: g for g in GOLDEN["cases"]}
    pairs = by["headings_and_long_text"]["model_calls"][0]["pairs"]
    assert any(p[1].startswith("Section ") and "\n" in p[1] for p in pairs)
    assert max(len(p[1]) for p in pairs) == 512 * 4                      # cut at max_length * 4 characters
    assert [r["original_rank"] for r in by["boosts_reorder"]["result"]][:2] == [1, 12]   # a boost moved chunk 1 above 12
    assert len(by["keep3_top_k_1"]["result"]) == 3 and len(by["keep3_top_k_0"]["result"]) == 3
    assert [r["chunk_id"] for r in by["exact_ties"]["result"]][:2] == ["chunk_003", "chunk_007"]
    assert by["model_raises"]["result"][0]["rerank_score"] == repr(1.0 / 1.2)     # fallback: similarity_score of the candidate


def test_selection_restatement_matches_fixture_scores():
    """select_host (what rdx_rerank_select computes) on the fixture's scores and recorded boosts"""
    for case, gold in zip(W.cases(), GOLDEN["cases"]):
        if case["raises"] or not case["idx"] or "raises" in gold:
            continue
        boosts = [float(b[2]) for b in gold["boosts"]] if gold["boosts"] else None
        order, final, count = RR.select_host(np.asarray(case["scores"], dtype=np.float32), boosts, case["top_k"], case["min_score"])
        assert [repr(final[i]) for i in order[:count]] == [r["rerank_score"] for r in gold["result"]], case["name"]
        assert order[:count] == [r["original_rank"] for r in gold["result"]], case["name"]


def test_interface_mirrors_reference():
    sig = inspect.signature(RR.CrossEncoderReranker.__init__)
    params = list(sig.parameters)[1:]
    assert params[:6] == ["model_name", "device", "batch_size", "max_length", "trust_remote_code", "min_score"]
    assert set(params[6:]) == {"dtype", "cache_dir"}
    assert {k: sig.parameters[k].default for k in params[:6]} == GOLDEN["defaults"]
    rs = inspect.signature(RR.CrossEncoderReranker.rerank)
    assert list(rs.parameters)[1:] == ["query", "chunks", "top_k", "topic_matcher", "question_topics"]
    assert rs.parameters["top_k"].default == 8 and rs.parameters["topic_matcher"].default is None
    assert list(RR.RankedChunk.__dataclass_fields__) == ["chunk_id", "text", "document_path", "rerank_score", "original_rank", "metadata"]
    r = RR.CrossEncoderReranker(cache_dir="/nonexistent")
    assert r.is_loaded is False and r.rerank("q", []) == [] and r.is_loaded is False     # nothing to rank: nothing loaded
    with pytest.raises(RuntimeError, match="never downloads"):
        r.rerank("q", case_chunks({"idx": [0]}))


def test_hash_pair_tokenizer_layout_and_longest_first():
    from rag_dpo_amd.embedding_provider import _HashTokenizer
    t = _HashTokenizer(1000)
    enc = t.pairs(["a b c", "a " * 300], ["d e", "x " * 50], 20)
    ids, att = enc["input_ids"].numpy(), enc["attention_mask"].numpy()
    assert att[0].sum() == 9 and list(ids[0, [0, 4, 5, 8]]) == [0, 2, 2, 2] and (ids[0, 9:] == 1).all()
    assert att[1].sum() == 20 and list(ids[1, [0, 9, 10, 19]]) == [0, 2, 2, 2]          # 16 pieces: 8 + 8
    enc = t.pairs(["a b c"], ["x " * 50], 20)
    assert list(enc["input_ids"].numpy()[0, [0, 4, 5, 19]]) == [0, 2, 2, 2]             # the short query is kept whole
    assert t(["a b c"])["input_ids"].tolist() == [[0] + enc["input_ids"].tolist()[0][1:4] + [2]]   # same piece ids as single texts


def hf_scores(model, tok_pairs, pairs):
    """transformers' XLMRobertaForSequenceClassification + sigmoid, one pair at a time (no padding involved), fp64 out"""
    out = []
    with torch.no_grad():
        for q, d in pairs:
            enc = tok_pairs([q], [d])
            n = int(enc["attention_mask"].sum())
            logit = model(input_ids=enc["input_ids"][:, :n]).logits.reshape(-1)[0]
            out.append(float(torch.sigmoid(logit.double())))
    return np.asarray(out)


def spread_head(model, scale=40.0):
    """a random-init head barely separates pairs (their <s> rows are alike): scaled, the scores spread while the fp32 error stays small"""
    with torch.no_grad():
        model.classifier.out_proj.weight.mul_(scale)


def test_packed_pair_forward_matches_module_forward_tiny():
    r = RR.CrossEncoderReranker("random-init:tiny")
    r.packed_forward = True
    r._load_model()
    m = r._model
    assert m.path == "cpu-packed"
    spread_head(m.model)
    pairs = [(W.QUERY, " ".join(f"w{i % 37}" for i in range(k))) for k in (1, 7, 30, 61, 140, 700)] + [("", "seul"), ("q " * 400, "d")]
    got = m.predict(pairs, batch_size=3)
    want = hf_scores(m.model, m.tokenize, pairs)
    assert got.dtype == np.float32 and got.shape == (len(pairs),)
    assert np.abs(got - want).max() <= 1e-5 and np.ptp(want) > 1e-3, (got, want)
    r2 = RR.CrossEncoderReranker("random-init:tiny")
    r2._load_model()
    assert r2._model.path == "cpu-module"
    spread_head(r2._model.model)
    assert np.abs(r2._model.predict(pairs, batch_size=3) - want).max() <= 1e-5          # padded batches of the module forward


def make_reranker_checkpoint(path, num_labels=1, arch="seqcls"):
    """an XLM-R sequence-classification checkpoint with a trained sentencepiece tokenizer, written to `path`"""
    import random
    import sentencepiece as spm
    from transformers import XLMRobertaConfig, XLMRobertaForSequenceClassification, XLMRobertaModel, XLMRobertaTokenizer
    os.makedirs(path, exist_ok=True)
    words = ("durée conservation données personnelles vidéosurveillance images caméras traitement registre responsable CNIL "
             "consentement cookies mois procédure délai Quelle Comment des de la le une est les sont au plus sauf").split()
    rnd = random.Random(1)
    txt = os.path.join(path, "corpus.txt")
    with open(txt, "w", encoding="utf-8") as f:
        for _ in range(2000):
            f.write(" ".join(rnd.choice(words) for _ in range(rnd.randint(4, 25))) + " ?\n")
    spm.SentencePieceTrainer.train(input=txt, model_prefix=os.path.join(path, "spm"), vocab_size=120, model_type="unigram",
                                   character_coverage=1.0, hard_vocab_limit=False, minloglevel=2)
    sp = spm.SentencePieceProcessor(model_file=os.path.join(path, "spm.model"))
    pieces = [(sp.id_to_piece(i), sp.get_score(i)) for i in range(sp.get_piece_size()) if not (sp.is_control(i) or sp.is_unknown(i))]
    vocab = [("<s>", 0.0), ("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0)] + pieces + [("<mask>", 0.0)]
    ckpt = os.path.join(path, "reranker-local")
    XLMRobertaTokenizer(vocab=vocab).save_pretrained(ckpt)
    torch.manual_seed(3)
    cfg = XLMRobertaConfig(vocab_size=len(vocab), hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                           max_position_embeddings=514, type_vocab_size=1, pad_token_id=1, bos_token_id=0, eos_token_id=2,
                           num_labels=num_labels)
    model = XLMRobertaForSequenceClassification(cfg) if arch == "seqcls" else XLMRobertaModel(cfg, add_pooling_layer=False)
    if arch == "seqcls":
        spread_head(model)
    model.save_pretrained(ckpt)
    return ckpt


def test_local_checkpoint_loads_and_scores(tmp_path):
    from transformers import AutoTokenizer, XLMRobertaForSequenceClassification
    ckpt = make_reranker_checkpoint(str(tmp_path))
    chunks = case_chunks({"idx": [0, 1, 2, 5, 9]})
    r = RR.CrossEncoderReranker(model_name="reranker-local", cache_dir=str(tmp_path), min_score=0.0)
    out = r.rerank(W.QUERY, chunks, top_k=5)
    assert r.is_loaded and r.last_rerank_stats["path"] == "cpu-module" and len(out) == 5
    tok = AutoTokenizer.from_pretrained(ckpt, local_files_only=True)
    model = XLMRobertaForSequenceClassification.from_pretrained(ckpt, local_files_only=True).eval()
    pairs = [(W.QUERY, (c.metadata["heading"] + "\n" + c.text if c.metadata.get("heading") else c.text)[:2048]) for c in chunks]
    want = hf_scores(model, lambda q, d: tok(q, d, truncation="longest_first", max_length=512, return_tensors="pt"), pairs)
    got = {o.original_rank: o.rerank_score for o in out}
    assert max(abs(got[i] - want[i]) for i in range(5)) <= 1e-5
    assert [o.original_rank for o in out] == sorted(range(5), key=lambda i: got[i], reverse=True)
    assert np.ptp(want) > 1e-3
    r2 = RR.CrossEncoderReranker(model_name=ckpt, min_score=0.0)          # the directory itself; the packed forward on the same pairs
    r2.packed_forward = True
    out2 = r2.rerank(W.QUERY, chunks, top_k=5)
    assert r2.last_rerank_stats["path"] == "cpu-packed"
    assert max(abs(a.rerank_score - got[a.original_rank]) for a in out2) <= 1e-5


def test_unsupported_checkpoints_raise(tmp_path):
    two = make_reranker_checkpoint(str(tmp_path / "two"), num_labels=2)
    with pytest.raises(ValueError, match="num_labels=2"):
        RR.CrossEncoderReranker(model_name=two).rerank("q", case_chunks({"idx": [0]}))
    base = make_reranker_checkpoint(str(tmp_path / "base"), arch="model")
    with pytest.raises(ValueError, match="architectures=\\['XLMRobertaModel'\\]"):
        RR.CrossEncoderReranker(model_name=base).rerank("q", case_chunks({"idx": [0]}))
    remote = tmp_path / "remote"                                          # what Jina's checkpoint looks like: custom code, never run
    remote.mkdir()
    (remote / "config.json").write_text(json.dumps({"model_type": "xlm-roberta", "architectures": ["XLMRobertaForSequenceClassification"],
                                                   "auto_map": {"AutoModelForSequenceClassification": "modeling.Custom"},
                                                   "num_labels": 1}))
    cfg = json.loads((remote / "config.json").read_text())
    cfg["model_type"] = "bert"
    (remote / "config.json").write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="model_type='bert'.*remote code|remote code.*model_type='bert'"):
        RR.CrossEncoderReranker(model_name=str(remote), trust_remote_code=True).rerank("q", case_chunks({"idx": [0]}))
    with pytest.raises(ValueError, match="unknown random-init spec"):
        RR.CrossEncoderReranker(model_name="random-init:huge").rerank("q", case_chunks({"idx": [0]}))


def test_entry_points_fail_with_code_and_message_without_gpu():
    from rag_dpo_amd import _lib
    L = _lib.load(require_gpu=False)
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    assert L.rdx_rerank_head_f16(0, p, 0, 64, p, p, p, p, p, p, None) == _lib.RDX_ERR_INVALID and "n must be" in _lib.last_error()
    assert L.rdx_rerank_head_f16(0, p, 1025, 64, p, p, p, p, p, p, None) == _lib.RDX_ERR_INVALID
    assert L.rdx_rerank_head_f16(0, p, 4, 96, p, p, p, p, p, p, None) == _lib.RDX_ERR_INVALID and "multiple of 64" in _lib.last_error()
    assert L.rdx_rerank_head_f16(0, p, 4, 8192, p, p, p, p, p, p, None) == _lib.RDX_ERR_INVALID
    assert L.rdx_rerank_head_f16(0, p, 4, 64, p, p, p, p, None, p, None) == _lib.RDX_ERR_INVALID and "null" in _lib.last_error()
    assert L.rdx_rerank_head_f16(0, p + 4, 4, 64, p, p, p, p, p, p, None) == _lib.RDX_ERR_INVALID and "aligned" in _lib.last_error()
    assert L.rdx_rerank_select(0, p, None, 0, 3, 0.08, 3, p, p, p, None) == _lib.RDX_ERR_INVALID and "n must be" in _lib.last_error()
    assert L.rdx_rerank_select(0, p, None, 4, -1, 0.08, 3, p, p, p, None) == _lib.RDX_ERR_INVALID and "top_k" in _lib.last_error()
    assert L.rdx_rerank_select(0, p, None, 4, 3, 0.08, -1, p, p, p, None) == _lib.RDX_ERR_INVALID
    assert L.rdx_rerank_select(0, p, None, 4, 3, 0.08, 3, None, p, p, None) == _lib.RDX_ERR_INVALID
    if not torch.cuda.is_available():                                     # valid arguments, no device: a HIP error, never a crash
        assert L.rdx_rerank_head_f16(0, p, 4, 64, p, p, p, p, p, p, None) not in (0, _lib.RDX_ERR_INVALID) and _lib.last_error()
        assert L.rdx_rerank_select(0, p, None, 4, 3, 0.08, 3, p, p, p, None) not in (0, _lib.RDX_ERR_INVALID) and _lib.last_error()


def test_documents_from_ranked_chunks_ignores_n_chunks_per_doc():
    ranked = [RR.RankedChunk(f"c{i}", "t", f"d{i % 2}", 0.9 - 0.1 * i, i, {"chunk_nature": "GUIDE"}) for i in range(5)]
    docs = documents_from_ranked_chunks(ranked, n_chunks_per_doc=1)
    assert [d.document_path for d in docs] == ["d0", "d1"] and [len(d.chunks) for d in docs] == [3, 2]
    assert docs[0].chunks[0].distance == 1.0 - 0.9 and docs[0].chunks[0].hybrid_score == 0.9 and docs[0].chunks[0].confidence == "medium"
    assert documents_from_ranked_chunks([]) == []

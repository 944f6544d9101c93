"""The world of tests/golden/reranker_golden.json: a pool of retrieved chunks, the scripted cross-encoder scores of each case and the
topic vectors a fake embedding provider hands to the reference's TopicMatcher. Shared by the maker (which runs the reference's
CrossEncoderReranker.rerank on it) and by the tests (which run rag_dpo_amd.reranker on the same inputs).

Documents carry one chunk nature each: RetrievedDocument.primary_nature is max(set(natures), key=natures.count), which decides a
tie by string-hash order."""
import numpy as np

QUERY = "Quelle est la durée de conservation des données de vidéosurveillance ?"
LONG_TEXT = " ".join(f"mot{i % 97} conservation" for i in range(700))      # ~9 000 characters: past max_length * 4 = 2048


def pool():
    """24 chunks over 6 documents: dicts with the RetrievedChunk fields the reranker reads"""
    docs = [("docs/cnil/videosurveillance.pdf", "GUIDE"), ("docs/cnil/conservation.html", "DOCTRINE"),
            ("docs/edpb/consent.pdf", "DOCTRINE"), ("docs/cnil/cookies.html", "GUIDE"), ("docs/rgpd/article5.txt", "TEXTE_LEGAL"),
            ("docs/entreprise/charte.docx", "PROCEDURE")]
    tags = ["durée de conservation, vidéosurveillance", "consentement", "cookies, traceurs", "", "sécurité des données",
            "consentement explicite", "archivage", "durée de conservation"]
    out = []
    for i in range(24):
        path, nature = docs[i % len(docs)]
        meta = {"document_path": path, "chunk_nature": nature, "chunk_index": i // len(docs), "confidence": ["high", "medium", "low"][i % 3]}
        if i % 4 == 1:
            meta["heading"] = f"Section {i}: conservation des images"
        if tags[i % len(tags)]:
            meta["rgpd_topics"] = tags[i % len(tags)]
        if i == 7:
            meta.pop("confidence")                     # documents_from_ranked_chunks defaults it to "medium"
        text = LONG_TEXT if i in (5, 17) else f"Chunk {i}: les images sont conservées {i % 5 + 1} mois au plus, sauf procédure."
        out.append({"chunk_id": f"chunk_{i:03d}", "text": text, "document_path": path, "metadata": meta, "distance": 0.2 + 0.025 * i})
    return out


def topic_vectors():
    """name -> unit vector (d = 64) with chosen cosines between topics and tags: exact names match without an embedding,
    'consentement explicite' ~ 'consentement' (0.9), 'traceurs' ~ 'cookies' (0.8), 'archivage' ~ 'durée de conservation'
    (0.6, under the 0.65 threshold: no boost)"""
    rng = np.random.default_rng(20261015)
    base = {}
    for name in ("consentement", "cookies", "durée de conservation", "vidéosurveillance", "sécurité des données"):
        v = rng.standard_normal(64)
        base[name] = v / np.linalg.norm(v)

    def near(a, c):
        u = rng.standard_normal(64)
        u -= base[a] * (base[a] @ u)
        u /= np.linalg.norm(u)
        return c * base[a] + np.sqrt(1 - c * c) * u
    base["consentement explicite"] = near("consentement", 0.9)
    base["traceurs"] = near("cookies", 0.8)
    base["archivage"] = near("durée de conservation", 0.6)
    return {k: [float(x) for x in v] for k, v in base.items()}


def _f32(xs):
    return [float(np.float32(x)) for x in xs]


def cases():
    """name, candidate indices into pool(), scripted float32 scores, top_k, min_score, question topics, raises"""
    rng = np.random.default_rng(7)
    f08 = float(np.float32(0.08))                      # 0.07999999821186066: under min_score = 0.08
    up = float(np.nextafter(np.float32(0.08), np.float32(1)))
    c = []
    add = lambda name, idx, scores, top_k=8, min_score=0.08, topics=None, raises=False: c.append(  # noqa: E731
        {"name": name, "idx": list(idx), "scores": _f32(scores), "top_k": top_k, "min_score": min_score, "topics": topics, "raises": raises})
    add("basic_40_candidates", list(range(24)) + list(range(16)), rng.uniform(0, 1, 40), top_k=10)
    add("exact_ties", range(12), [0.5, 0.25, 0.5, 0.9, 0.25, 0.5, 0.1, 0.9, 0.05, 0.5, 0.25, 0.01], top_k=6)
    add("ties_with_duplicate_ids", [3, 3, 4, 4, 5], [0.3, 0.3, 0.7, 0.7, 0.3], top_k=4)
    add("straddling_min_score", range(9), [f08, up, 0.0801, 0.0799, 0.5, 0.08, 0.081, 0.079, 0.2], top_k=9)
    add("keep3_top_k_1", range(6), [0.01, 0.02, 0.03, 0.04, 0.05, 0.06], top_k=1)
    add("keep3_top_k_2", range(6), [0.01, 0.9, 0.03, 0.04, 0.05, 0.06], top_k=2)
    add("keep3_top_k_3", range(6), [0.01, 0.02, 0.03, 0.04, 0.05, 0.06], top_k=3)
    add("keep3_one_above", range(7), [0.01, 0.02, 0.5, 0.04, 0.05, 0.06, 0.07], top_k=8)
    add("keep3_top_k_0", range(5), [0.4, 0.3, 0.2, 0.1, 0.6], top_k=0)
    add("top_k_beyond_n", range(5), [0.2, 0.4, 0.1, 0.3, 0.5], top_k=20)
    add("n_0", [], [], top_k=8)
    add("n_1", [2], [0.7], top_k=8)
    add("n_2", [1, 2], [0.3, 0.6], top_k=8)
    add("n_2_one_below", [1, 2], [0.03, 0.6], top_k=8)
    add("n_2_all_below", [1, 2], [0.03, 0.06], top_k=8)          # the reference raises IndexError in its closing log line
    add("n_3_all_below", [1, 2, 3], [0.03, 0.06, 0.01], top_k=8)
    add("headings_and_long_text", [1, 5, 9, 13, 17, 0], [0.4, 0.8, 0.6, 0.2, 0.9, 0.1], top_k=4)
    add("boosts_reorder", range(16), [0.50, 0.52, 0.45, 0.40, 0.55, 0.41, 0.44, 0.39, 0.2, 0.3, 0.35, 0.38, 0.6, 0.1, 0.05, 0.07],
        top_k=8, topics=["consentement", "cookies"])
    add("boosts_lift_over_min_score", range(8), [0.01, 0.02, 0.07, 0.075, 0.03, 0.079, 0.02, 0.06], top_k=5,
        topics=["durée de conservation", "sécurité des données"])
    add("boosts_empty_topics", range(8), [0.3, 0.2, 0.5, 0.1, 0.4, 0.6, 0.7, 0.05], top_k=5, topics=[])
    add("model_raises", range(10), [0.5] * 10, top_k=4, raises=True)
    add("model_raises_top_k_beyond_n", range(3), [0.5] * 3, top_k=8, raises=True)
    return c

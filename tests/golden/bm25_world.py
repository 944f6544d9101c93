"""The seeded French-like world shared by make_bm25_golden.py (capture, drives the IMPORTED reference bm25_index.py and
RAGRetriever in the build container) and the BM25 tests (replay, this repo's code only): a few thousand chunks with
metadata and embeddings, the summaries, and the queries of every case."""
import json
import os
import zlib

import numpy as np

from rag_dpo_amd import synth
from rag_dpo_amd.collection import Collection

N, DIM, DOCS = 3000, 64, 150
NAT = ["GUIDE", "DOCTRINE", "SANCTION", "TECHNIQUE"]
DOMAIN = ["conservation", "vidéosurveillance", "sous-traitant", "article", "28", "consentement", "cookies", "registre",
          "traitements", "transfert", "union", "européenne", "sanction", "amende", "cœur", "œuvre", "données-sensibles",
          "sécurité", "délégué", "violation", "notification", "72", "heures", "employeur", "salariés", "badge", "biométrie",
          "prospection", "commerciale", "mineurs", "santé", "recherche", "anonymisation", "pseudonymisation", "durée"]
SYL = ["con", "ser", "va", "tion", "trai", "te", "ment", "pro", "tec", "sé", "cu", "ri", "té", "lé", "gi", "ti", "mi", "ré",
       "gis", "tre", "da", "no", "ca", "pi", "ta", "lu", "fé", "ô", "bi", "zo"]
STOP = ["le", "la", "les", "de", "des", "du", "et", "à", "l", "d", "en", "pour", "est", "qui"]


def _vocab():
    rng = np.random.default_rng(7)
    words = list(DOMAIN)
    while len(words) < 900:
        w = "".join(rng.choice(SYL, size=int(rng.integers(2, 5))))
        if w not in words:
            words.append(w)
    return words


def chunk_texts():
    rng = np.random.default_rng(11)
    words = _vocab()
    p = 1.0 / np.arange(1, len(words) + 1) ** 1.05
    p /= p.sum()
    texts = []
    for i in range(N):
        if i % 211 == 5:
            texts.append("   " if i % 2 else "")                      # blank: skipped by the index
            continue
        if i % 211 == 17:
            texts.append("le la de l'à d'en")                        # no token: skipped
            continue
        if i % 97 == 0 and i:
            texts.append(texts[-1])                                   # exact duplicate: ties
            continue
        n = int(rng.integers(15, 80))
        toks = list(rng.choice(words, size=n, p=p))
        toks += list(rng.choice(STOP, size=n // 3))
        if rng.random() < 0.62:
            toks.append("données")                                    # in more than half the rows: epsilon idf
        rng.shuffle(toks)
        t = " ".join(toks)
        if i % 13 == 0:
            t = t.capitalize() + " — Article 28, l'Employeur"
        texts.append(t)
    return texts


def metadatas():
    out = []
    for i in range(N):
        m = {"document_path": f"cnil/doc_{(i * 7) % DOCS:03d}.html", "chunk_nature": NAT[i % 4], "chunk_index": i % 9,
             "confidence": "high" if i % 3 else "medium", "source": "ENTREPRISE" if i % 11 == 0 else "CNIL"}
        if i % 5 == 0:
            m["source_url"] = ("https://www." if i % 2 else "http://") + f"cnil.fr/page_{(i * 7) % DOCS % 40}"
        if i % 29 == 3:
            del m["document_path"]                                    # no path: the "" group
        out.append(m)
    return out


def build_collection(engine_factory):
    col = Collection("rag_dpo_chunks", metadata={"hnsw:space": "cosine"}, engine_factory=engine_factory)
    col.add(ids=[f"chunk_{i:05d}" for i in range(N)], documents=chunk_texts(), embeddings=synth.make_corpus(N, DIM).tolist(),
            metadatas=metadatas())
    return col


def summaries():
    rng = np.random.default_rng(5)
    words = _vocab()
    out = {}
    for d in range(DOCS):
        path = f"cnil/doc_{d:03d}.html"
        if d % 23 == 4:
            out[path] = {"document_title": f"Titre {d}", "summary": "ERREUR: génération impossible", "source_url": ""}
        elif d % 23 == 9:
            out[path] = {"document_title": f"Titre {d}", "summary": "", "source_url": "https://cnil.fr/x"}
        elif d % 23 == 15:
            out[path] = {"document_title": "le", "summary": "de la les", "source_url": ""}   # no token: skipped
        else:
            body = " ".join(rng.choice(words[:300], size=int(rng.integers(20, 60))))
            out[path] = {"document_title": f"Fiche {d} {words[d % 35]}", "summary": f"NATURE: GUIDE. SUJETS: {body}",
                         "source_url": f"https://www.cnil.fr/fr/{words[(d * 3) % 35]}-{d}"}
    return out


def write_summaries(directory):
    """the summaries file SummaryBM25Index.build reads (generated, not committed) -> its path"""
    path = os.path.join(directory, "document_summaries.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(summaries(), f, ensure_ascii=False, sort_keys=True)
    return path


class HashEmbedder:
    """stands in for EmbeddingProvider: deterministic text -> vector near some corpus row"""
    model_name = "hash-embedder"

    def __init__(self, poison_sub=()):
        self.c = synth.make_corpus(N, DIM)
        self.calls = []
        self.poison_sub = tuple(poison_sub)

    def embed(self, texts):
        self.calls.append(list(texts))
        out = []
        for t in texts:
            if any(p in t for p in self.poison_sub):
                out.append([float("nan")] * DIM)      # collection.query raises on it -> that sub-query is skipped
                continue
            h = zlib.crc32(t.encode("utf-8"))
            v = self.c[h % N] + 0.8 * np.random.default_rng(h).standard_normal(DIM).astype(np.float32)
            out.append((v / np.linalg.norm(v)).astype(np.float32).tolist())
        return out


def expander(question):
    """stands in for QueryExpander.expand: original first, then 3 reformulations"""
    return [question, question + " obligations employeur", "sanction " + question, question.lower() + " durée conservation"]


TOKENIZER_TEXTS = [
    "Quelle est la durée de conservation des données de vidéosurveillance ?",
    "L'article 28 du règlement : le sous-traitant et l'employeur",
    "ŒUVRE, cœur, Æsir, ex-æquo, naïve, maïs, Noël, où, déjà, très, même, être, été",
    "données-sensibles -- tiret- -début fin- a-b-c 72-heures 2024-05",
    "C'est l'avis n°2 d'un DPO (RGPD, art. 35) : J'y vais, qu'il m'a dit.",
    "   ", "", "x y z 1 2 à é", "MAJUSCULES ACCENTUÉES ÉTÉ ÇA",
]

# (query, top_k, doc_filter: None | "empty" | list of paths)
CHUNK_CASES = [
    ("durée de conservation des données de vidéosurveillance", 50, None),
    ("registre des traitements sous-traitant article 28", 30, None),
    ("consentement consentement cookies", 40, None),                     # duplicate query token
    ("zzzinconnu conservation qqqabsent", 25, None),                     # out-of-vocabulary tokens
    ("le la les de", 30, None),                                          # tokenises to nothing
    ("zzzinconnu", 30, None),                                            # only unknown tokens
    ("données", 30, None),                                               # the epsilon-idf term: ties by row
    ("convavament vatrainoser", 4000, None),                             # top_k above the rows with a positive score
    ("biométrie badge salariés", 1, None),
    ("sécurité des données de santé", 50, "empty"),
    ("sécurité des données de santé", 50, ["cnil/doc_003.html", "cnil/doc_010.html", "cnil/doc_077.html", "absent/doc.html"]),
    ("transfert union européenne", 40, ["cnil/doc_042.html", ""]),
    ("Article 28, l'Employeur", 30, None),
]

SUMMARY_QUERIES = [("conservation vidéosurveillance", 20), ("consentement cookies prospection", 5), ("le la", 20),
                   ("zzzinconnu", 20), ("registre traitements", 200)]

Q0 = "Quelle est la durée de conservation des données de vidéosurveillance ?"
RETRIEVER_QUERIES = [
    {"query": Q0, "where": None, "n_candidates": 40, "prefilter": True, "expand": True, "poison_sub": []},
    {"query": "registre des traitements du sous-traitant article 28", "where": {"chunk_nature": {"$in": ["GUIDE", "DOCTRINE"]}},
     "n_candidates": 30, "prefilter": False, "expand": True, "poison_sub": []},
    {"query": "notification d'une violation en 72 heures", "where": None, "n_candidates": 30, "prefilter": True, "expand": False,
     "poison_sub": []},
    # sub-queries whose collection.query raises (NaN embedding): the reference skips their dense AND BM25 searches
    {"query": Q0, "where": None, "n_candidates": 30, "prefilter": True, "expand": True, "poison_sub": ["sanction "]},
    {"query": Q0, "where": None, "n_candidates": 30, "prefilter": True, "expand": True, "poison_sub": ["Quelle est"]},  # all but one
]

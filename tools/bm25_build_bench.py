"""Building a BM25 index from text: the host build (tokenize_french + Bm25Model, the default) against the device build
(rag_dpo_amd/bm25_build.py: k_bm25_tok / k_bm25_vocab) on the same synthetic French-like text, one JSON line per
size and side, appended to --out.

Text: a Zipf vocabulary of 200 000 words made of syllables (accents included), about 120 words per row of which a third are stop
words, some capitalised, some behind an elided article (l'…), some followed by a comma, some hyphenated. Sizes: 16 919 rows (the
reference's collection), 100 000, 1 M and 10 M. The two builds alternate, `--reps` times each up to 100 000 rows (medians) and once above,
and the arrays of the two models are compared (post_off, post_row, post_tf, idf, denom, the vocabulary in order) wherever both ran.
The host build of a size is skipped when the rate of the size before says it would take longer than --host-limit-s; at 10 M only
the device runs, and the line says how long the host was allowed.

Stages, seconds: host = tokenise | postings + statistics (Bm25Model) | rdx_bm25_create; device = encode (str.encode and the row
table, on the host) | upload | tokenise | sort + run lengths + vocabulary | download | host statistics | rdx_bm25_create.

    python tools/bm25_build_bench.py [--sizes 16919,100000] [--reps 3] [--host-limit-s 600] [--out profiles/bm25_build/ab.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402

from rag_dpo_amd import bm25  # noqa: E402
from rag_dpo_amd.bm25_build import DeviceBm25Builder  # noqa: E402

SYL = ["con", "ser", "va", "tion", "trai", "te", "ment", "pro", "tec", "sé", "cu", "ri", "té", "lé", "gi", "ti", "mi", "ré", "gis",
       "tre", "da", "no", "ca", "pi", "ta", "lu", "fé", "ô", "bi", "zo", "œu", "çon", "naï", "où", "è", "dû"]
VOCAB = 200_000


def surface_forms():
    rng = np.random.default_rng(7)
    words = set()
    while len(words) < VOCAB:
        words.add("".join(rng.choice(SYL, size=int(rng.integers(2, 6)))))
    words = np.array(sorted(words), dtype=object)
    rng.shuffle(words)
    hyphen = np.array([a + "-" + b for a, b in zip(words, np.roll(words, 1))], dtype=object)
    forms = [words, np.array([w.capitalize() for w in words], dtype=object), np.array([w + "," for w in words], dtype=object),
             np.array(["l'" + w for w in words], dtype=object), hyphen, np.array([w.upper() + "." for w in words], dtype=object)]
    return np.concatenate(forms + [np.array(sorted(bm25.STOPWORDS), dtype=object)])


def make_texts(n_rows, forms, seed, slab=250_000):
    """slab by slab, so that the generator's temporaries stay small beside the texts themselves"""
    n_stop = len(bm25.STOPWORDS)
    texts = []
    for first in range(0, n_rows, slab):
        rng = np.random.default_rng((seed, first))
        lens = rng.integers(60, 181, size=min(slab, n_rows - first))
        total = int(lens.sum())
        ids = (rng.zipf(1.15, size=total) - 1) % VOCAB
        form = rng.choice(6, size=total, p=[0.80, 0.05, 0.05, 0.04, 0.03, 0.03])
        pick = form * VOCAB + ids
        stop = rng.random(total) < 0.33
        pick[stop] = 6 * VOCAB + rng.integers(0, n_stop, size=int(stop.sum()))
        texts += [" ".join(x) for x in np.split(forms[pick], np.cumsum(lens)[:-1])]
    return texts


def host_build(texts):
    t0 = time.perf_counter()
    tokens = [t for t in map(bm25.tokenize_french, texts) if t]
    t1 = time.perf_counter()
    model = bm25.Bm25Model(tokens)
    t2 = time.perf_counter()
    eng = bm25.HipBm25(model.arrays(), 0)
    t3 = time.perf_counter()
    eng.close()
    return model, {"tokenise": t1 - t0, "postings_and_statistics": t2 - t1, "rdx_bm25_create": t3 - t2, "total": t3 - t0}


def device_build(texts, builder):
    t0 = time.perf_counter()
    _, model = builder.build(texts)
    t1 = time.perf_counter()
    eng = bm25.HipBm25(model.arrays(), 0)
    t2 = time.perf_counter()
    eng.close()
    T = dict(builder.timings)
    return model, {"encode_and_upload": T["upload"], "tokenise": T["tokenise"], "sort_rle_vocab": T["sort_rle"], "download": T["download"],
                   "host_statistics": T["host_stats"], "rdx_bm25_create": t2 - t1, "total": t2 - t0, "table_retries": builder.retries}


def equal(a, b):
    return (list(a.term_id) == list(b.term_id) and all(np.array_equal(getattr(a, n), getattr(b, n)) and
                                                       getattr(a, n).tobytes() == getattr(b, n).tobytes()
                                                       for n in ("post_off", "post_row", "post_tf", "idf", "denom")))


def median(rows):
    return {k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16919,100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-limit-s", type=float, default=600.0)
    ap.add_argument("--table-slots", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm25_build", "ab.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    forms = surface_forms()
    builder = DeviceBm25Builder(0, table_slots=args.table_slots)
    builder.build(make_texts(2000, forms, 0))                      # warm-up: the library, torch's allocator, the sort's workspace
    host_s_per_row = 0.0

    def emit(rec):
        line = json.dumps(rec, ensure_ascii=False)
        print(line, flush=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")

    for n_rows in map(int, args.sizes.split(",")):
        t = time.perf_counter()
        texts = make_texts(n_rows, forms, n_rows)
        gen_s = round(time.perf_counter() - t, 2)
        run_host = n_rows < 10_000_000 and host_s_per_row * n_rows <= args.host_limit_s
        reps = args.reps if n_rows <= 100_000 else 1
        hosts, devs, same = [], [], None
        for _ in range(reps):                                       # the two builds alternate
            if run_host:
                hm, ht = host_build(texts)
                hosts.append(ht)
            dm, dt = device_build(texts, builder)
            devs.append(dt)
            if run_host:
                same = equal(dm, hm) and (same is None or same)
                assert same, "the device-built index differs from the host-built one"
                del hm
        shape = {"rows": n_rows, "characters": sum(map(len, texts)), "terms": dm.n_terms, "postings": int(dm.post_off[-1]),
                 "tokens": int(dm.doc_len.sum()), "generate_s": gen_s, "reps": reps}
        if run_host:
            emit({**shape, "side": "host", **median(hosts)})
            host_s_per_row = median(hosts)["total"] / n_rows
        else:
            emit({**shape, "side": "host", "skipped": True, "allowed_s": args.host_limit_s,
                  "extrapolated_s": round(host_s_per_row * n_rows, 1) if host_s_per_row else None})
        emit({**shape, "side": "device", **median(devs), "arrays_equal_host": same})
        del texts, dm

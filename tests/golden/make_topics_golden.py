#!/usr/bin/env python3
"""Captures tests/golden/topics_golden.json by running the reference's OWN TopicMatcher (src/utils/rgpd_topics.py, imported from a
reference checkout, never copied) over the scripted embedder and the cases of tests/golden/topics_world.py: per case the boost of
every candidate (topic_boost) and the similarity of every (topic, distinct tag) pair (similarity), as reprs of Python floats.
The JSON it writes is the committed fixture; the reference is needed only to regenerate it.

    python tests/golden/make_topics_golden.py <reference checkout>
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import topics_world as W  # noqa: E402


def main(reference):
    sys.path.insert(0, reference)
    from src.utils.rgpd_topics import TopicMatcher          # the reference

    out = {"generator": "tests/golden/make_topics_golden.py: the reference's TopicMatcher over tests/golden/topics_world.py", "cases": []}
    for case in W.cases():
        emb = W.ScriptedEmbedder(case["world"]) if case["world"] else None
        tm = TopicMatcher(embedding_provider=emb)
        boosts = [tm.topic_boost(case["topics"], s, threshold=case["threshold"]) for s in case["tags"]]
        tags = list(dict.fromkeys(t.strip() for s in case["tags"] if s for t in s.split(",") if t.strip()))
        sims = {topic: {tag: repr(float(tm.similarity(topic, tag))) for tag in tags} for topic in case["topics"]}
        if not case["exact"]:
            # the tests allow |d sim| <= dim * 2^-53 * sum |a_i b_i| between two summation orders: no similarity of such a case may
            # lie that close to the threshold, or a boost could be 0.0 under one order and positive under the other
            vec = W.WORLDS[case["world"]]
            for topic in case["topics"]:
                for tag in tags:
                    if tag in vec:
                        a, b = np.asarray(vec[topic]), np.asarray(vec[tag])
                        bound = len(a) * 2.0 ** -53 * float(np.abs(a * b).sum())
                        assert abs(float(sims[topic][tag]) - case["threshold"]) > 4 * bound, (case["name"], topic, tag)
        out["cases"].append({"name": case["name"], "boosts": [repr(float(b)) for b in boosts], "similarities": sims})
    with open(os.path.join(HERE, "topics_golden.json"), "w") as f:
        json.dump(out, f, indent=1, ensure_ascii=False)
    hits = {c["name"]: sum(1 for b in c["boosts"] if float(b) > 0) for c in out["cases"]}
    print(f"{len(out['cases'])} cases; boosted candidates: {hits}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

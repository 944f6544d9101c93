"""The scripted world of tests/golden/topics_golden.json: a seeded embedder (every value an fp32 number, as this project's providers
return them) and the cases the reference's TopicMatcher was run on (make_topics_golden.py). Shared by the generator and the tests."""
import numpy as np

T32 = float(np.float32(0.65))                       # the fp32 number next to the default threshold 0.65 (it lies below it)
T32_UP = float(np.nextafter(np.float32(0.65), np.float32(1.0)))
RAISES = "tag-qui-leve"                             # the embedder raises for this text
BIG_DIM = 96                                        # not a multiple of 64, more than one element per lane
BIG_TOPICS = ["cookies", "durée de conservation", "sous-traitance"]


def _d4():
    v = {
        "e1": [1.0, 0.0, 0.0, 0.0],
        "seuil": [T32, 0.0, 0.0, 0.0],               # e1 . seuil = T32 exactly
        "au-dessus": [T32_UP, 0.0, 0.0, 0.0],
        "opposé": [-1.0, 0.0, 0.0, 0.0],
        "nan": [float("nan"), 0.0, 0.0, 0.0],
        "nan2": [0.0, float("nan"), 0.0, 0.0],
        "cookies": [0.0, 0.0, 1.0, 0.0],
        "u1": [1.0, 2.0 ** -26, 0.0, 0.0],           # u1 . u2 = 1 + 2^-52 exactly: one ulp above 1.0
        "u2": [1.0, 2.0 ** -26, 0.0, 0.0],
        "moitié": [0.0, 0.0, 0.75, 0.0],
    }
    return v


def _big():
    rng = np.random.default_rng(20240611)
    unit = lambda x: (x / np.linalg.norm(x)).astype(np.float32)   # noqa: E731
    v = {}
    for t in BIG_TOPICS:
        v[t] = unit(rng.standard_normal(BIG_DIM))
    # tags at a spread of cosines to their topic: well below, around and well above the threshold (the generator asserts that none
    # lies within the summation-order bound of it)
    for k, t in enumerate(BIG_TOPICS):
        for j, cos in enumerate((0.2, 0.5, 0.6, 0.7, 0.8, 0.9, 0.97)):
            noise = rng.standard_normal(BIG_DIM)
            noise -= noise @ v[t].astype(np.float64) * v[t]
            noise /= np.linalg.norm(noise)
            v[f"tag-{k}-{j}"] = unit(cos * v[t].astype(np.float64) + (1 - cos * cos) ** 0.5 * noise)
    for j in range(6):
        v[f"bruit-{j}"] = unit(rng.standard_normal(BIG_DIM))
    return {k: [float(x) for x in x32] for k, x32 in v.items()}


WORLDS = {"d4": _d4(), "big": _big()}


class ScriptedEmbedder:
    """embed(texts) -> the world's vectors as lists of Python floats; raises for RAISES and for a text the world does not know"""

    def __init__(self, world: str):
        self.vec = WORLDS[world]
        self.calls = []

    def embed(self, texts):
        self.calls.append(list(texts))
        if RAISES in texts:
            raise RuntimeError("scripted embed failure")
        return [list(self.vec[t]) for t in texts]


def _question40():
    rng = np.random.default_rng(7)
    names = [k for k in WORLDS["big"] if k not in BIG_TOPICS]
    tags = []
    for c in range(40):
        k = int(rng.integers(0, 4))
        pick = [names[int(i)] for i in rng.integers(0, len(names), k)]
        if c == 5:
            pick = ["Cookies", pick[0] if pick else "bruit-0"]          # an exact match in a long question
        if c == 9:
            pick = [RAISES, "tag-1-5"]
        tags.append(", ".join(pick))
    return tags


def cases():
    """name, world (None: no embedder), topics, the candidates' tag strings, threshold, exact (the golden similarity comes from an
    exact match or from d <= 4 vectors with exact arithmetic: boosts compare bit for bit)"""
    d = 0.65
    return [
        dict(name="no topics", world="d4", topics=[], tags=["e1", "cookies, e1"], threshold=d, exact=True),
        dict(name="empty and whitespace-only tag strings", world="d4", topics=["e1"], tags=["", "   ", " , ,, ", None], threshold=d, exact=True),
        dict(name="exact match ignoring case, no embedder", world=None, topics=["Cookies", "droit d'accès"],
             tags=["cookies", "traceurs, COOKIES ", "traceurs", "Droit d'Accès,x", ""], threshold=d, exact=True),
        dict(name="exact match ignoring case, with embedder", world="d4", topics=["Cookies", "e1"], tags=["moitié, cookies", "COOKIES", "moitié"],
             threshold=d, exact=True),
        dict(name="an embed that raises for one tag", world="d4", topics=["e1", "cookies"], tags=[RAISES, f"{RAISES}, e1", f"u1, {RAISES}", "moitié"],
             threshold=d, exact=True),
        dict(name="fp32(0.65) lies below the default threshold", world="d4", topics=["e1"], tags=["seuil", "au-dessus"], threshold=d, exact=True),
        dict(name="similarity exactly at the threshold", world="d4", topics=["e1"], tags=["seuil"], threshold=T32, exact=True),
        dict(name="similarity just above the threshold", world="d4", topics=["e1"], tags=["au-dessus", "seuil, au-dessus"], threshold=T32, exact=True),
        dict(name="negative similarity", world="d4", topics=["e1"], tags=["opposé", "opposé, moitié"], threshold=d, exact=True),
        dict(name="NaN vector", world="d4", topics=["e1", "nan2"], tags=["nan", "nan, au-dessus", "seuil, nan", "nan, u1"], threshold=T32, exact=True),
        dict(name="one ulp above 1.0 before an exact match in a later topic", world="d4", topics=["u1", "cookies"], tags=["u2, Cookies", "u2"],
             threshold=d, exact=True),
        dict(name="one ulp above 1.0 after an exact match in an earlier topic", world="d4", topics=["cookies", "u1"], tags=["u2, Cookies", "Cookies, u2"],
             threshold=d, exact=True),
        dict(name="one ulp above 1.0, then an exact match under the same topic", world="d4", topics=["u1"], tags=["u2, U1", "U1, u2", "u2, e1"],
             threshold=d, exact=True),
        dict(name="40 candidates, 3 topics, repeated tags", world="big", topics=list(BIG_TOPICS), tags=_question40(), threshold=d, exact=False),
    ]

"""TEST-ONLY: the grouped search's definition (rag_dpo_amd/groups.py) as a literal double loop, and the expected answer
of a collection computed from the ORACLE's exact scores — never from a second call into the code under test; and k_group_select's
position table as a sequential walk, with the lists of colliding codes the GPU tests cut."""
import numpy as np

from oracle import oracle as O
from rag_dpo_amd.where import kind_of


def group_key(v):
    """what makes two metadata values one group: equal and of the same kind (1 and True differ); None = the row has no group"""
    return None if v is None else (kind_of(v), v)


def literal_groups(ranked_scores, ranked_rows, key_of_row, G, m):
    """walk the ranking; -> [(key, [(score, row), ...])]: the first G distinct keys met, each with its first m rows"""
    groups = []
    for s, r in zip(ranked_scores, ranked_rows):
        if r < 0:
            continue
        key = key_of_row[r]
        if key is None:
            continue
        for k2, members in groups:
            if k2 == key:
                if len(members) < m:
                    members.append((s, int(r)))
                break
        else:
            if len(groups) < G:
                groups.append((key, [(s, int(r))]))
    return groups


# ---- k_group_select's position table (csrc/group_kernel.hpp, step 2) restated on the host ---------------------------------------
# The constants are the header's: tests/test_group_table_model.py reads them out of the source and compares.
GROUP_TABLE = 8192
GROUP_MAX_K = 4096
HASH_MULT = 0x9E3779B1
HASH_SHIFT = 19
CODE_LIMIT = 1 << 20          # the collision lists' global codes stay below this (a group_off of 8 MB)


def home_slot(code):
    """group_slot0: the uint32 product's top 13 bits"""
    return ((int(code) * HASH_MULT) & 0xFFFFFFFF) >> HASH_SHIFT


def home_slots(codes):
    """home_slot of an array of codes >= 0"""
    return (((np.asarray(codes).astype(np.uint64) * np.uint64(HASH_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(HASH_SHIFT)).astype(np.int64)


def table_slots(codes_in_list_order):
    """insert the list's codes one after the other (negative: no group) -> {code: (slot, probes, wrapped)}. The kernel inserts in
    parallel: WHICH code of a chain gets which slot depends on who wins the CAS there; that the chain forms does not."""
    key, where = {}, {}
    for c in codes_in_list_order:
        c = int(c)
        if c < 0 or c in where:
            continue
        s, probes, wrapped = home_slot(c), 0, False
        while s in key:
            nxt = (s + 1) & (GROUP_TABLE - 1)
            wrapped = wrapped or nxt < s
            s, probes = nxt, probes + 1
            assert probes < GROUP_TABLE, "the table is full"
        key[s] = c
        where[c] = (s, probes, wrapped)
    return where


def table_walk(codes_in_list_order):
    """-> (displaced, longest_probe, wraps): codes that do not sit in their home slot, the most steps one code took, and the codes
    whose walk went from slot GROUP_TABLE - 1 on to slot 0"""
    w = table_slots(codes_in_list_order).values()
    return sum(1 for _, p, _ in w if p), max((p for _, p, _ in w), default=0), sum(1 for _, _, wr in w if wr)


_BY_HOME = {}


def codes_with_home(slot, below):
    """every code in [0, below) whose home slot is `slot`, ascending"""
    if below not in _BY_HOME:
        h = home_slots(np.arange(below))
        order = np.argsort(h, kind="stable")
        _BY_HOME[below] = (order, np.searchsorted(h[order], np.arange(GROUP_TABLE + 1)))
    order, start = _BY_HOME[below]
    return order[start[slot]: start[slot + 1]].copy()


def select_threads(k):
    """the workgroup k_group_select runs a list of k entries with (csrc/rdx_group.hip); thread t inserts positions t, t + NT, ..."""
    return 256 if k <= 1024 else 1024


class ListSpec:
    """one ranked list of the collision batch: the GLOBAL code of each of its k rows, its length, and what it claims to make the
    table do — claims that tests/test_group_table_model.py checks against table_walk"""

    def __init__(self, name, codes, count=None, claims=()):
        self.name, self.codes, self.count, self.claims = name, np.asarray(codes, dtype=np.int64), count, frozenset(claims)

    def listed(self):
        return self.codes[: len(self.codes) if self.count is None else self.count]


_COLLISION_LISTS = {}


def collision_lists(k):
    """The lists tests/test_gpu_group_kernels.py cuts at list length k: at most a dozen, codes in [0, CODE_LIMIT). Claims:
    'displaced' some code leaves its home slot; 'wraps' a walk goes from the last slot to slot 0; 'long' one code takes >= 64
    steps; 'same_thread' colliding codes sit at positions one thread inserts one after the other; 'winner_last' the first group's
    code ends the chain when the race goes to the later positions."""
    if k in _COLLISION_LISTS:
        return _COLLISION_LISTS[k]
    rng = np.random.default_rng(4181 + k)
    pick = lambda slot, n: rng.permutation(codes_with_home(slot, CODE_LIMIT))[:n]                # noqa: E731
    tile = lambda seq: np.resize(np.asarray(seq, dtype=np.int64), k)                             # noqa: E731  (position i: seq[i % len])
    long_if = lambda n: ("long",) if n - 1 >= 64 else ()                                         # noqa: E731
    out = []
    # one home slot: the members of min(k, 100) codes interleave, so positions of different codes contend inside one wave
    n1 = min(k, 100)
    for h in (0, 4000, GROUP_TABLE - 1):
        out.append(ListSpec(f"one_home_{h}", tile(pick(h, n1)), claims=("displaced",) + long_if(n1) + (("wraps",) if h == GROUP_TABLE - 1 else ())))
    # a chain across the wrap: c codes each at the last two slots and at slot 0, in three orders
    c = min(100, k // 3)
    chain = np.concatenate([pick(GROUP_TABLE - 2, c), pick(GROUP_TABLE - 1, c), pick(0, c)])
    chain_claims = ("displaced", "wraps") + long_if(3 * c - 2)
    shuffled = rng.permutation(chain)
    out.append(ListSpec("chain_ascending", tile(chain), claims=chain_claims))
    out.append(ListSpec("chain_reversed", tile(chain[::-1]), claims=chain_claims))
    out.append(ListSpec("chain_shuffled", tile(shuffled), claims=chain_claims))
    # the winner at the end of the chain: the first group's home is slot 0, which the codes of the last two slots flood through;
    # its other members come back every 7 positions of the list's first half, and every other code has a row in the second half
    flood = min(c - 1, k // 4)
    others = np.concatenate([pick(GROUP_TABLE - 2, flood), pick(GROUP_TABLE - 1, flood)])
    first = pick(0, 1)[0]
    winner = tile(rng.permutation(others))
    winner[: k // 2: 7] = first
    out.append(ListSpec("winner_last", winner, claims=("displaced", "wraps", "winner_last") + long_if(2 * flood)))
    # same-thread collisions: the positions t, t + NT, t + 2 NT, t + 3 NT of every thread t hold distinct codes of one home slot
    # (homes 8 slots apart: no chain reaches the next thread's)
    nt = select_threads(k)
    if k > nt:
        same = np.empty(k, dtype=np.int64)
        for t in range(min(nt, k - nt)):
            at = np.arange(t, k, nt)
            same[at] = pick((8 * t + 5) % GROUP_TABLE, len(at))
        lone = np.arange(min(nt, k - nt), nt)                                                    # threads with one position
        same[lone] = [pick((8 * t + 5) % GROUP_TABLE, 1)[0] for t in lone]
        out.append(ListSpec("same_thread", same, claims=("displaced", "same_thread")))
    # sparse random: min(k, 4096) distinct codes below CODE_LIMIT, then the same codes 1 - 8 times each
    sparse = rng.choice(CODE_LIMIT, size=min(k, GROUP_MAX_K), replace=False)
    sparse_claims = ("displaced",) if k >= 1024 else ()                                          # (64 codes over 8192 slots rarely collide)
    out.append(ListSpec("sparse", tile(sparse), claims=sparse_claims))
    out.append(ListSpec("sparse_repeated", rng.permutation(np.repeat(sparse, rng.integers(1, 9, size=len(sparse))))[:k], claims=sparse_claims))
    # chains with holes: a third of the shuffled chain's rows carry no key; the same in a list that is not full
    holes = tile(shuffled)
    holes[rng.permutation(k)[: k // 3]] = -1
    out.append(ListSpec("chain_holes", holes, claims=("displaced", "wraps")))
    out.append(ListSpec("chain_holes_not_full", holes, count=k - 1, claims=("displaced", "wraps")))
    assert len(out) <= 12 and all(s.codes.shape == (k,) and s.codes.max() < CODE_LIMIT for s in out)
    for s in out:
        s.codes.setflags(write=False)
    _COLLISION_LISTS[k] = out
    return out


def check_claims(spec):
    """a list's claims against the sequential walk of its listed codes; -> (displaced, longest_probe, wraps)"""
    listed = spec.listed()
    displaced, longest, wraps = table_walk(listed)
    present = np.unique(listed[listed >= 0])
    # at most one code per home slot is not displaced, whatever the order of insertion
    assert displaced >= len(present) - len(np.unique(home_slots(present))), spec.name
    if "displaced" in spec.claims:
        assert displaced > 0, spec.name
    if "wraps" in spec.claims:
        assert wraps > 0, spec.name
    if "long" in spec.claims:
        assert longest >= 64, (spec.name, longest)
    if "same_thread" in spec.claims:
        nt, k = select_threads(len(spec.codes)), len(spec.codes)
        pairs = [(i, i + nt) for i in range(k - nt)]
        assert pairs and all(spec.codes[i] != spec.codes[j] and home_slot(spec.codes[i]) == home_slot(spec.codes[j]) for i, j in pairs), spec.name
    if "winner_last" in spec.claims:
        first = int(listed[listed >= 0][0])
        assert table_slots(listed)[first][1] == 0                                  # in list order the first group's code is at home,
        late = table_slots(listed[::-1])                                           # when the later positions win every race, every
        assert late[first][1] == len(late) - 3 > 0, spec.name                      # other code but two lies between its home and its slot
    return displaced, longest, wraps


def oracle_ranking(corpus_hat, q_raw, allow=None):
    """the whole ranking of the allowed rows per query: (scores f32 [nq][n], rows i64 [nq][n], counts i32 [nq])"""
    return O.cosine_topk(corpus_hat, q_raw, corpus_hat.shape[0], allow)


def expected(corpus_hat, q_raw, values, G, m, allow=None):
    """per query [(value, [row, ...], [score bits, ...], [distance, ...])] from the oracle's ranking; values[r] = the key's value or None"""
    keys = [group_key(v) for v in values]
    s, r, c = oracle_ranking(corpus_hat, q_raw, allow)
    out = []
    for b in range(s.shape[0]):
        gs = literal_groups(s[b, : c[b]], r[b, : c[b]], keys, G, m)
        out.append([(key[1], [row for _, row in mem], [int(np.float32(sc).view(np.uint32)) for sc, _ in mem],
                     [float(np.float32(1.0) - np.float32(sc)) for sc, _ in mem]) for key, mem in gs])
    return out


def as_expected(res, col):
    """a query_groups result in expected()'s shape: rows from ids, score bits unknown (None), distances as returned"""
    out = []
    for b in range(len(res["ids"])):
        out.append([(res["groups"][b][g], col.rows_of(res["ids"][b][g]), None, res["distances"][b][g]) for g in range(len(res["ids"][b]))])
    return out


def same(got, want):
    """groups, their order, rows, their order and the distances' bits"""
    assert len(got) == len(want)
    for b, (gq, wq) in enumerate(zip(got, want)):
        assert [(type(v), v) for v, _, _, _ in gq] == [(type(v), v) for v, _, _, _ in wq], f"query {b}: groups"
        for (v, gr, _, gd), (_, wr, _, wd) in zip(gq, wq):
            assert gr == wr, f"query {b} group {v!r}: rows {gr} != {wr}"
            assert np.asarray(gd, dtype=np.float32).tobytes() == np.asarray(wd, dtype=np.float32).tobytes(), f"query {b} group {v!r}: distances"

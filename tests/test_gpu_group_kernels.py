"""GPU: the grouped search's two kernels called directly (rag_dpo_amd.engine.group_select / group_fill), bit for bit against the
definition as a literal loop (tests/groups_model.py) and the oracle's exact scores.

k_group_select: list lengths around the wave (63, 64, 65), around the switch between its two workgroup widths (1024, 1025) and the
largest (4096); each with the smallest, the default and the largest (groups, rows per group); and, since the dense codes of those
lists never collide in its position table, codes chosen by home slot (test_select_on_colliding_codes). k_group_fill: dims whose float4 groups
sit around one and four per lane and beyond the register path (1028), with the job spans (around a wave's 64 listed rows and the
workgroup's 256), masks and ties the header names."""
import numpy as np
import pytest

import groups_model as GM

pytestmark = pytest.mark.gpu


# ---- k_group_select --------------------------------------------------------------------------------------------------------------
class Lists:
    """a batch of ranked lists over one row -> group table; every query owns a disjoint range of rows, and (add) a disjoint range of
    codes or (add_global) whatever codes it names"""

    def __init__(self, k):
        self.k = k
        self.scores, self.rows, self.counts = [], [], []
        self.row_code = []          # the table, row by row
        self.next_code = 0

    def add(self, codes, count=None, scores=None, extra=None):
        """codes: the code of each of the k listed rows, LOCAL to this query (-1: no group); count: the list's length; extra: {local
        code: unlisted rows of that group elsewhere in the collection}"""
        k = self.k
        codes = np.asarray(codes, dtype=np.int64)
        assert codes.shape == (k,)
        base = len(self.row_code)
        glob = np.where(codes >= 0, codes + self.next_code, -1)
        self.row_code += glob.tolist()
        n_local = int(codes.max()) + 1 if (codes >= 0).any() else 0
        for c, more in (extra or {}).items():
            n_local = max(n_local, c + 1)
            self.row_code += [c + self.next_code] * more
        self.next_code += n_local
        self._list(base, count, scores)

    def add_global(self, codes, count=None, scores=None):
        """codes: the GLOBAL code of each of the k listed rows (-1: no group). A code may recur in another query: a group's size is
        its rows in the whole table."""
        codes = np.asarray(codes, dtype=np.int64)
        assert codes.shape == (self.k,) and codes.min() >= -1
        base = len(self.row_code)
        self.row_code += codes.tolist()
        self.next_code = max(self.next_code, int(codes.max()) + 1)
        self._list(base, count, scores)

    def _list(self, base, count, scores):
        k = self.k
        count = k if count is None else count
        rows = np.arange(base, base + k, dtype=np.int64)
        rows[count:] = -1
        sc = np.linspace(0.9, -0.9, k, dtype=np.float32) if scores is None else np.asarray(scores, dtype=np.float32)
        sc = sc.copy()
        sc[count:] = -np.inf
        self.scores.append(sc)
        self.rows.append(rows)
        self.counts.append(count)

    def tables(self):
        rg = np.asarray(self.row_code, dtype=np.int32)
        off = np.zeros(self.next_code + 1, dtype=np.int64)
        np.cumsum(np.bincount(rg[rg >= 0], minlength=self.next_code), out=off[1:])
        return rg, off


def run_select(L, G, m, only=None):
    """only: a slice of the batch's lists to run alone, over the same tables"""
    import torch
    from rag_dpo_amd import engine as E
    dev = torch.device("cuda", 0)
    rg, off = L.tables()
    s, r, c = np.stack(L.scores), np.stack(L.rows), np.asarray(L.counts, dtype=np.int32)
    if only is not None:
        s, r, c = (np.ascontiguousarray(a[only]) for a in (s, r, c))
    t = lambda a: torch.from_numpy(a).to(dev)
    out = {k: v.cpu().numpy() for k, v in E.group_select(t(s), t(r), t(c), t(rg), t(off), G, m).items()}
    return out, (s, r, c, rg, off)


def check_select(out, inputs, G, m):
    s, r, c, rg, off = inputs
    k = s.shape[1]
    assert out["bad"].tolist() == [0]
    keys = [None if x < 0 else int(x) for x in rg]
    for b in range(s.shape[0]):
        n = int(c[b])
        want = GM.literal_groups(s[b, :n], r[b, :n], keys, G, m)
        listed = {}
        for row in r[b, :n]:
            if row >= 0 and rg[row] >= 0:
                listed[int(rg[row])] = listed.get(int(rg[row]), 0) + 1
        full = n == k
        assert out["found"][b] == len(want), b
        assert out["short"][b] == int(full and len(listed) < G), b
        for g in range(G):
            if g >= len(want):
                assert out["code"][b, g] == -1 and out["count"][b, g] == 0 and out["complete"][b, g] == 1
                assert (out["row"][b, g] == -1).all() and np.isneginf(out["score"][b, g]).all()
                continue
            code, mem = want[g]
            assert out["code"][b, g] == code, (b, g)
            assert out["count"][b, g] == len(mem)
            assert out["row"][b, g, : len(mem)].tolist() == [row for _, row in mem], (b, g)
            assert out["score"][b, g, : len(mem)].tobytes() == np.asarray([x for x, _ in mem], dtype=np.float32).tobytes()
            assert (out["row"][b, g, len(mem):] == -1).all() and np.isneginf(out["score"][b, g, len(mem):]).all()
            size = int(off[code + 1] - off[code])
            assert out["complete"][b, g] == int(not full or listed[code] >= min(m, size)), (b, g, listed[code], size)


DEFINITION_K = [1, 63, 64, 65, 1024, 1025, 4096]
GROUPS_AND_SIZES = [(1, 1), (5, 3), (64, 16)]


def definition_lists(k, G):
    """the batch of test_select_matches_the_definition (tests/test_group_table_model.py walks it through the table's model: every
    query's codes are a dense range, which never collides)"""
    rng = np.random.default_rng(k * 100 + G)
    L = Lists(k)
    L.add(rng.integers(-1, max(2, k // 3), size=k))                               # many groups, some rows without one
    L.add(rng.integers(0, 70, size=k) if k > 70 else rng.integers(0, 3, size=k), extra={0: 5, 1: 40})
    L.add(np.zeros(k))                                                             # all rows in one group
    L.add(np.zeros(k), extra={0: 100})
    L.add(np.arange(k))                                                            # every row its own group
    front = np.arange(k) % 7
    front[: k // 3] = -1
    front[k - k // 4:] = -1                                                        # rows without a group at the front and at the end
    L.add(front)
    L.add(rng.integers(0, 9, size=k), count=k // 2)                                # a list that is not full
    L.add(rng.integers(0, 9, size=k), count=0)                                     # an empty one
    L.add(rng.integers(0, 9, size=k), scores=np.full(k, 0.25))                     # equal scores: the list's (row) order stands
    L.add(rng.integers(0, 9, size=k), scores=np.where(np.arange(k) % 2 == 0, 0.0, -0.0))
    if k >= G:                                                                     # the short flag's boundary: G - 1 and G groups in a full list
        if G > 1:
            L.add(np.arange(k) % (G - 1))
        L.add(np.arange(k) % G)
        L.add(np.minimum(np.arange(k), G - 1))                                     # the G-th group appears at the last possible moment
        L.add(np.maximum(np.arange(k) - (k - G), 0))                               # ... and G groups whose last G - 1 close the list
    return L


@pytest.mark.parametrize("G,m", GROUPS_AND_SIZES)
@pytest.mark.parametrize("k", DEFINITION_K)
def test_select_matches_the_definition(k, G, m):
    L = definition_lists(k, G)
    out, inputs = run_select(L, G, m)
    check_select(out, inputs, G, m)


@pytest.mark.parametrize("G,m", GROUPS_AND_SIZES)
@pytest.mark.parametrize("k", [64, 65, 1024, 1025, 4096])
def test_select_on_colliding_codes(k, G, m):
    """The position table's probing path, which dense codes never enter (tests/test_group_table_model.py): codes below 2^20 chosen by
    home slot (GM.collision_lists: one home slot, chains across the wrap from the last slot to slot 0, the first group at the end of
    a chain, collisions inside one thread, sparse random codes, chains with keyless rows and a list that is not full). Which code
    gets which slot depends on who wins a CAS; the outputs must not: every output equals the literal loop's, a second run and a
    run of one list alone return the same bytes."""
    specs = GM.collision_lists(k)
    L = Lists(k)
    seen = set()
    for spec in specs:
        displaced, longest, wraps = GM.check_claims(spec)                           # the branch the list is built for is really taken
        seen |= {name for name, hit in (("displaced", displaced > 0), ("wraps", wraps > 0), ("long", longest >= 64)) if hit}
        L.add_global(spec.codes, count=spec.count)
    assert {"displaced", "wraps"} <= seen and (k < 100 or "long" in seen)
    out, inputs = run_select(L, G, m)
    check_select(out, inputs, G, m)
    again, _ = run_select(L, G, m)
    for name in out:
        assert again[name].tobytes() == out[name].tobytes(), name
    j = [spec.name for spec in specs].index("chain_shuffled")
    alone, _ = run_select(L, G, m, only=slice(j, j + 1))
    for name in ("row", "score", "count", "code", "complete", "found", "short"):
        assert alone[name][0].tobytes() == out[name][j].tobytes(), name
    assert alone["bad"].tolist() == [0]


@pytest.mark.parametrize("k", [64, 4096])
@pytest.mark.parametrize("m", [1, 3, 16])
def test_select_complete_flag_boundary(k, m):
    """a group with m - 1, m, m + 1 listed rows against a group size of exactly that many and of more"""
    L = Lists(k)
    for listed in (m - 1, m, m + 1):
        if listed < 1:
            continue
        for unlisted in (0, 1, 50):
            codes = np.full(k, 1)
            codes[np.arange(listed) * (k // (listed + 1))] = 0                     # group 0's rows, spread over the list
            assert (codes == 0).sum() == listed
            L.add(codes, extra={0: unlisted})
            L.add(codes, extra={0: unlisted}, count=k - 1)                         # not full: complete whatever is listed
    out, inputs = run_select(L, 2, m)
    check_select(out, inputs, 2, m)
    assert 1 in out["complete"] and (m == 1 or 0 in out["complete"])               # both sides of the boundary were met


def test_select_refuses_rows_and_codes_outside_the_tables():
    import torch
    from rag_dpo_amd import engine as E
    dev = torch.device("cuda", 0)
    k, G, m = 64, 3, 2
    L = Lists(k)
    L.add(np.arange(k) % 5)
    rg, off = L.tables()
    s, c = np.stack(L.scores), np.asarray(L.counts, dtype=np.int32)
    t = lambda a: torch.from_numpy(a).to(dev)
    rows = np.stack(L.rows)
    rows[0, 1] = len(rg)                                                           # one past the table: never read
    out = {kk: v.cpu().numpy() for kk, v in E.group_select(t(s), t(rows), t(c), t(rg), t(off), G, m).items()}
    assert out["bad"].tolist() == [1]
    as_padding = rows.copy()
    as_padding[0, 1] = -1
    ref = {kk: v.cpu().numpy() for kk, v in E.group_select(t(s), t(as_padding), t(c), t(rg), t(off), G, m).items()}
    assert ref["bad"].tolist() == [0]
    for name in ("row", "score", "count", "code", "found"):
        assert out[name].tobytes() == ref[name].tobytes(), name
    wild = rg.copy()
    wild[2] = len(off) - 1                                                         # a code the offsets do not cover
    assert E.group_select(t(s), t(np.stack(L.rows)), t(c), t(wild), t(off), G, m)["bad"].item() == 1
    ok = (t(s), t(np.stack(L.rows)), t(c), t(rg), t(off))
    for G_, m_ in ((0, 1), (65, 1), (1, 0), (1, 17)):
        with pytest.raises(ValueError):
            E.group_select(*ok, G_, m_)
    big = torch.zeros((1, 4097), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        E.group_select(big, torch.zeros((1, 4097), dtype=torch.int64, device=dev), t(c), t(rg), t(off), 1, 1)


# ---- k_group_fill -----------------------------------------------------------------------------------------------------------------
N_ROWS = 4300
M_FILL = 5


def fill_world(dim):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    x[100:140] = x[7]                                                              # exact copies: equal scores, the row id decides
    x[4200:4210] = x[7]
    q = rng.standard_normal((3, dim)).astype(np.float32)
    q[1] = x[7] + 0.01 * rng.standard_normal(dim).astype(np.float32)               # the copies are this query's best rows
    return x, q


def want_fill(scores, rows, allow, m):
    rows = [int(r) for r in rows if allow is None or allow[r]]
    rows.sort(key=lambda r: (-float(scores[r]), r))
    return rows[:m]


@pytest.mark.parametrize("dim", [4, 252, 256, 260, 1020, 1024, 1028])
def test_fill_matches_the_oracle(dim, oracle):
    import torch
    from rag_dpo_amd import engine as E
    O = oracle
    x, q = fill_world(dim)
    ix = E.HipIndex(dim)
    ix.add(x)
    dev = torch.device("cuda", 0)
    xh, qh = O.normalize_rows(x), O.normalize_rows(q)
    scores = [O.scores(xh, qh[b]) for b in range(q.shape[0])]
    rng = np.random.default_rng(1)
    group_rows = np.concatenate([np.arange(4096), np.arange(4096, N_ROWS), np.sort(rng.choice(N_ROWS, 500, replace=False)), np.arange(90, 150)])
    m = M_FILL
    spans = [(0, 0), (5, 5), (0, 1), (4100, 4101), (10, 10 + m - 1), (10, 10 + m), (10, 10 + m + 1), (0, 4096), (4096, N_ROWS), (N_ROWS, N_ROWS + 500),
             (N_ROWS + 500, N_ROWS + 560), (N_ROWS + 3, N_ROWS + 131), (60, 60 + 64), (60, 60 + 65), (61, 61 + 63),
             (200, 200 + 255), (200, 200 + 256), (200, 200 + 257), (90, 90 + 129)]        # around one and four waves' worth of listed rows
    jq, jb, je = [], [], []
    for b in range(q.shape[0]):
        for a, e in spans:
            jq.append(b)
            jb.append(a)
            je.append(e)
    alternate = np.arange(N_ROWS) % 2 == 0
    few = np.zeros(N_ROWS, dtype=bool)
    few[[7, 101, 4205, 3000]] = True
    gq, gr = torch.from_numpy(q).to(dev), torch.from_numpy(group_rows).to(dev)
    for allow in (None, alternate, few, np.zeros(N_ROWS, dtype=bool)):
        mask = ix.make_mask(O.pack_mask(allow, N_ROWS)) if allow is not None else None
        for mm in ((m, 1, 16) if allow is None else (m,)):
            sc, ro, cn = (t.cpu().numpy() for t in E.group_fill(ix, gq, jq, jb, je, gr, mm, mask=mask))
            assert sc.shape == (len(jq), mm) and ro.shape == (len(jq), mm)
            for j in range(len(jq)):
                want = want_fill(scores[jq[j]], group_rows[jb[j]: je[j]], allow, mm)
                assert cn[j] == len(want), (j, allow is None)
                assert ro[j, : len(want)].tolist() == want, (dim, j, jb[j], je[j])
                assert sc[j, : len(want)].tobytes() == scores[jq[j]][want].tobytes(), (dim, j)          # the oracle's bits
                assert (ro[j, len(want):] == -1).all() and np.isneginf(sc[j, len(want):]).all()
        if mask is not None:
            mask.close()
    if dim == 256:
        # rows the index does not hold are skipped, never read
        odd_rows = torch.tensor([5, -1, N_ROWS, 1 << 40, 6], dtype=torch.int64, device=dev)
        sc, ro, cn = E.group_fill(ix, gq, [0], [0], [5], odd_rows, 4)
        assert cn.tolist() == [2] and sorted(ro[0, :2].tolist()) == [5, 6]
        for bad in (dict(job_query=[3]), dict(job_query=[-1]), dict(job_begin=[2], job_end=[1]), dict(job_end=[len(group_rows) + 1]),
                    dict(job_begin=[0], job_end=[4097]), dict(group_size=0), dict(group_size=17)):
            args = dict(job_query=[0], job_begin=[0], job_end=[4], group_size=3)
            args.update(bad)
            with pytest.raises(ValueError):
                E.group_fill(ix, gq, args["job_query"], args["job_begin"], args["job_end"], gr, args["group_size"])
        sc, ro, cn = E.group_fill(ix, gq, [], [], [], gr, 3)                        # no jobs: nothing to do
        assert cn.numel() == 0
    ix.close()

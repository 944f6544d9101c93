"""CPU tests of the position table's model in tests/groups_model.py (home_slot, table_walk, codes_with_home, collision_lists), which
tests/test_gpu_group_kernels.py::test_select_on_colliding_codes and tests/test_gpu_groups.py replay through k_group_select.

  * the hash's multiplier and shift, the table's size and the list's largest length are the ones in csrc/group_kernel.hpp, read out
    of the source: a kernel change that moves a home slot fails here instead of un-aiming the GPU tests;
  * the finding that made those tests necessary, as assertions: the multiplier is the Fibonacci constant, so dense codes (what
    GroupTables hands out, and what every list of test_select_matches_the_definition holds) never leave their home slots below
    4182 of them — the probing path (another code in the slot, the step, the wrap) was not executed by any test;
  * per list of the collision batch, the branch it claims is really taken, from the walk itself."""
import os
import re

import numpy as np
import pytest

import groups_model as GM
import test_gpu_group_kernels as TG

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rag_dpo_amd", "csrc")


def test_constants_are_the_header_s():
    src = open(os.path.join(CSRC, "group_kernel.hpp")).read()
    const = lambda name: [int(v) for v in re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)]   # noqa: E731
    assert const("GROUP_TABLE") == [GM.GROUP_TABLE] == [8192]
    assert const("GROUP_MAX_K") == [GM.GROUP_MAX_K] == [4096]
    assert GM.GROUP_MAX_K * 2 <= GM.GROUP_TABLE                     # at most GROUP_MAX_K codes: a probe always meets an empty slot
    flat = re.sub(r"\s+", " ", src)
    m = re.search(r"int group_slot0\(int32_t code\) \{ return \(int\)\(\(\(uint32_t\)code \* (0x[0-9A-Fa-f]+)u\) >> (\d+)\); \}", flat)
    assert m, "group_slot0 changed: restate it in groups_model.home_slot"
    assert (int(m.group(1), 16), int(m.group(2))) == (GM.HASH_MULT, GM.HASH_SHIFT)
    assert 1 << (32 - GM.HASH_SHIFT) == GM.GROUP_TABLE              # the shift leaves exactly the table's index bits
    assert "s = (s + 1) & (GROUP_TABLE - 1);" in flat               # the probe step the walk restates
    rdx_group = re.sub(r"\s+", " ", open(os.path.join(CSRC, "rdx_group.hip")).read())
    assert "if (k <= 1024) hipLaunchKernelGGL(k_group_select<256>," in rdx_group                # select_threads
    assert "else hipLaunchKernelGGL(k_group_select<1024>," in rdx_group
    assert (GM.select_threads(1024), GM.select_threads(1025)) == (256, 1024)


def test_home_slot_and_walk_by_hand():
    assert GM.home_slot(0) == 0 and GM.home_slot(1) == 0x9E3779B1 >> 19
    assert GM.home_slot(3) == ((3 * 0x9E3779B1) % 2 ** 32) >> 19    # the product wraps in uint32
    codes = np.random.default_rng(0).integers(0, GM.CODE_LIMIT, size=500)
    assert GM.home_slots(codes).tolist() == [GM.home_slot(c) for c in codes]
    for slot in (0, 4000, 8191):
        got = GM.codes_with_home(slot, 50_000)
        assert got.tolist() == [c for c in range(50_000) if GM.home_slot(c) == slot] and len(got) >= 5
    assert GM.table_walk([]) == GM.table_walk([-1, -1]) == (0, 0, 0)
    assert GM.table_walk([7, 7, -1, 7]) == (0, 0, 0)
    a, b, c = GM.codes_with_home(8191, GM.CODE_LIMIT)[:3]
    z = GM.codes_with_home(0, GM.CODE_LIMIT)[1]
    assert GM.table_walk([a, b]) == (1, 1, 1)                       # b: 8191 -> 0
    assert GM.table_walk([a, b, a, c, b]) == (2, 2, 2)              # c: 8191 -> 0 -> 1
    assert GM.table_walk([a, b, z]) == (2, 1, 1)                    # z's home is taken by b: displaced without a wrap
    assert GM.table_slots([z, a, b])[b] == (1, 2, True)


def test_dense_codes_never_collide_below_4182():
    """what GroupTables numbers (0, 1, 2, ... by first appearance) stays in its home slots until code 4181 meets code 0"""
    homes = GM.home_slots(np.arange(4182))
    assert len(np.unique(homes[:4181])) == 4181
    assert homes[4181] == homes[0] == 0 and GM.codes_with_home(0, 5000).tolist() == [0, 4181]
    assert GM.table_walk(range(4181)) == (0, 0, 0) and GM.table_walk(range(4182)) == (1, 1, 0)
    for base in (0, 1000, 5000, 12345):                             # any range of GROUP_MAX_K consecutive codes
        assert GM.table_walk(range(base, base + GM.GROUP_MAX_K)) == (0, 0, 0), base


@pytest.mark.parametrize("G,m", TG.GROUPS_AND_SIZES)
@pytest.mark.parametrize("k", TG.DEFINITION_K)
def test_the_definition_batch_never_probes(k, G, m):
    """every list test_select_matches_the_definition cuts keeps every code in its home slot: that test cannot tell a wrong probe"""
    L = TG.definition_lists(k, G)
    rg, _ = L.tables()
    assert len(L.rows) >= 10
    for rows, count in zip(L.rows, L.counts):
        assert GM.table_walk(rg[rows[:count]]) == (0, 0, 0)


@pytest.mark.parametrize("k", [64, 65, 1024, 1025, 4096])
def test_every_collision_list_takes_its_branch(k):
    specs = GM.collision_lists(k)
    names = [s.name for s in specs]
    assert len(set(names)) == len(names) <= 12
    want = {"one_home_0", "one_home_4000", "one_home_8191", "chain_ascending", "chain_reversed", "chain_shuffled", "winner_last",
            "sparse", "sparse_repeated", "chain_holes", "chain_holes_not_full"} | ({"same_thread"} if k > GM.select_threads(k) else set())
    assert set(names) == want
    by = dict(zip(names, specs))
    walks = {s.name: GM.check_claims(s) for s in specs}
    for s in specs:
        assert s.codes.shape == (k,) and s.codes.min() >= -1 and s.codes.max() < GM.CODE_LIMIT
        assert "displaced" in s.claims or s.name.startswith("sparse")
    n1, c = min(k, 100), min(100, k // 3)
    for h in (0, 4000, 8191):                                       # n1 codes of one home: a chain of n1 slots whatever the order
        s = by[f"one_home_{h}"]
        assert len(np.unique(s.codes)) == n1 and set(GM.home_slots(s.codes)) == {h}
        assert walks[s.name] == (n1 - 1, n1 - 1, n1 - 1 if h == 8191 else 0)
        assert len(set(s.codes[:64].tolist())) == min(64, n1)       # different codes inside the first wave
    for name in ("chain_ascending", "chain_reversed", "chain_shuffled"):
        s = by[name]
        assert sorted(np.bincount(GM.home_slots(np.unique(s.codes)), minlength=GM.GROUP_TABLE)[[8190, 8191, 0]]) == [c] * 3
        displaced, longest, wraps = walks[name]
        # 3c codes of three adjacent homes fill slots 8190, 8191, 0 .. 3c - 3 in any order of insertion: whoever holds the last slot
        # came at least 3c - 3 steps, and of the 2c codes of the last two slots only two can stay there
        assert displaced >= 3 * c - 3 and longest >= 3 * c - 3 and wraps >= 2 * c - 2
    # ascending homes: only the first code stays at home; the last code of slot 0 ends the chain; all but two of the 2c codes wrap
    assert walks["chain_ascending"] == (3 * c - 1, 3 * c - 3, 2 * c - 2)                       # (299, 297, 198) with 300 codes
    assert sorted(by["chain_ascending"].codes[: 3 * c].tolist()) == sorted(by["chain_reversed"].codes[: 3 * c].tolist()) \
        == sorted(by["chain_shuffled"].codes[: 3 * c].tolist())
    assert by["chain_ascending"].codes.tolist() != by["chain_shuffled"].codes.tolist()
    if k >= 1024:                                                   # the lists long enough for 300 codes: probes beyond one wave's width
        assert c == 100 and all("long" in by[n].claims for n in ("chain_ascending", "chain_reversed", "chain_shuffled", "winner_last", "one_home_8191"))
        assert all(walks[n][0] > 0 for n in ("sparse", "sparse_repeated"))
        assert len(np.unique(by["sparse"].codes)) == min(k, GM.GROUP_MAX_K) and by["sparse"].codes.max() >= 2 ** 19
        rep = np.bincount(np.unique(by["sparse_repeated"].codes, return_inverse=True)[1])
        assert rep.max() > 1 and set(by["sparse_repeated"].codes.tolist()) <= set(by["sparse"].codes.tolist())
    holes, short = by["chain_holes"], by["chain_holes_not_full"]
    assert (holes.codes < 0).sum() == k // 3 and short.count == k - 1 and holes.count is None and (short.codes == holes.codes).all()
    assert set(holes.codes[holes.codes >= 0].tolist()) <= set(by["chain_shuffled"].codes.tolist())
    first = by["winner_last"].codes[0]
    assert GM.home_slot(first) == 0 and (by["winner_last"].codes == first).sum() >= 2
    if "same_thread" in by:
        nt, s = GM.select_threads(k), by["same_thread"]
        assert len(np.unique(s.codes)) == k                         # every position its own group: any two that meet are different codes
        assert walks["same_thread"][0] == k - nt                    # thread t's first code stays at home, its later ones are displaced


def test_sparse_codes_collide_as_measured():
    """production reaches the probing path as soon as a key has more values than 4181: a list of 4096 distinct codes out of 12 000
    dense ones (tests/test_gpu_groups.py builds such a collection). Over these 20 draws the walk gives 528 displaced codes at
    least (median 571) and probes of up to 17 steps; asserted is only that every draw probes."""
    walks = [GM.table_walk(np.random.default_rng(s).choice(12_000, size=4096, replace=False)) for s in range(20)]
    assert all(displaced > 0 and longest > 1 for displaced, longest, _ in walks)

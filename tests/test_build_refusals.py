"""CPU: rag_dpo_amd.build.refusals — which resource records build_lib refuses, by message, for the product and for a variant build.
The records are hand-made: one readable, spill-free entry per kernel, exactly the least count of every family."""
import copy

import pytest

from rag_dpo_amd import build

CLEAN = {"vgprs": 32, "agprs": 0, "spill_vgprs": 0, "spill_sgprs": 0, "scratch_bytes": 0, "lds_bytes": 0}
# family -> (its kernels in a clean record, the opening of the message a spilling kernel brings, refused in a variant build as well)
FAMILIES = {
    "scan": ([f"k_scan_v{i}" for i in range(16)], "scan kernels spill registers", True),
    "docs": ([f"k_docs_{i}" for i in range(4)], "the where_document kernels (doc_kernel.hpp) spill or were not found", True),
    "meta": (["k_meta_eval", "k_meta_fill"], "the `where` predicate kernels (meta_kernel.hpp) spill or were not found", True),
    # the two single-question topic kernels are the only ones of "k_topic" that are not batched kernels too
    "topic": (["k_topic_simsEPK", "k_topic_replayEPK"], "the topic boost kernels (topic_kernel.hpp) spill or were not found", True),
    "batch": (["k_topic_sims_batch", "k_topic_replay_batch"] + [f"k_rerank_select_batchILi{w}E" for w in (64, 256, 1024)],
              "the batched reranker kernels (rerank_batch_kernel.hpp) spill or were not found", True),
    "space": ([f"k_space_{i}" for i in range(5)], "the ip / l2 space kernels (space_kernel.hpp) spill or were not found", True),
    "fuse": (["k_fuse_rrf"], "the rank fusion kernel (fuse_kernel.hpp) spills or was not found", True),
    "refine": (["k_refine", "k_refine_spill"], "the refine kernels (refine_kernel.hpp) spill or were not found", False),
    "attention": (["k_enc_attention_mfma"], "k_enc_attention_mfma no longer fits its occupancy target without spilling", False),
    "gemm": ([f"k_enc_gemm_{i}" for i in range(6)], "k_enc_gemm kernels spill or use scratch", False),
}
UNREAD_SCAN = "the compiler's resource remarks could not be read for the scan kernels"
UNREAD_GEMM = "the compiler's resource remarks could not be read for the k_enc_gemm kernels (6 found)"


def clean_record() -> dict:
    res = {k: dict(CLEAN) for kernels, _, _ in FAMILIES.values() for k in kernels}
    res["k_rerank_head"] = dict(CLEAN)          # a kernel no check names
    return res


def heads(messages):
    return [m.split(" — refused")[0] for m in messages]


@pytest.mark.parametrize("variant", [False, True])
def test_a_clean_record_is_not_refused(variant):
    assert build.refusals(clean_record(), variant) == []


def test_the_table_holds_the_least_counts():
    least = {c.fragments[0]: c.least for c in build.SPILL_CHECKS if c.least}
    assert least == {"k_scan": 16, "k_docs": 4, "k_meta": 2, "k_topic": 2, "k_rerank_select_batch": 5, "k_space": 5, "k_fuse": 1,
                     "k_refine": 2, "k_enc_gemm": 6}
    assert [c.fragments[0] for c in build.SPILL_CHECKS if not c.variant] == ["k_refine", "k_enc_attention_mfma", "k_enc_gemm"]


@pytest.mark.parametrize("figure", [("spill_vgprs", 1), ("scratch_bytes", 8)])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_spilling_kernel_is_refused_by_its_family_s_message(family, figure):
    kernels, message, in_variant = FAMILIES[family]
    res = clean_record()
    res[kernels[-1]][figure[0]] = figure[1]
    expect = [message]
    got = build.refusals(res, variant=False)
    assert heads(got) == expect
    assert f"  {kernels[-1]}: " in got[0] and str(res[kernels[-1]]) in got[0]      # the message names the kernel and its figures
    assert heads(build.refusals(res, variant=True)) == (expect if in_variant else [])


def test_a_batched_topic_kernel_answers_to_both_of_its_families():
    res = clean_record()
    res["k_topic_replay_batch"]["spill_vgprs"] = 1
    assert heads(build.refusals(res)) == [FAMILIES["topic"][1], FAMILIES["batch"][1]]


def test_a_spill_message_lists_the_family_or_the_offenders():
    res = clean_record()
    res["k_docs_3"]["spill_vgprs"] = 1
    res["k_scan_v2"]["scratch_bytes"] = 8
    scan, docs = build.refusals(res)
    assert scan.count("\n  k_scan") == 1 and "\n  k_scan_v2: " in scan          # the offenders alone
    assert docs.count("\n  k_docs") == 4                                         # the family as found


@pytest.mark.parametrize("variant", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_family_a_kernel_short_is_refused(family, variant):
    kernels, message, in_variant = FAMILIES[family]
    res = clean_record()
    del res[kernels[0]]
    expect = {"scan": [UNREAD_SCAN], "attention": [], "topic": [],               # (three batched topic kernels remain: k_topic still has its 2)
              "gemm": ["the compiler's resource remarks could not be read for the k_enc_gemm kernels (5 found)"],
              }.get(family, [message])
    if variant and family == "refine":
        expect = []
    assert heads(build.refusals(res, variant)) == expect


@pytest.mark.parametrize("variant", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_an_entry_lacking_the_keys_is_refused_where_the_check_would_be_blind(family, variant):
    kernels, message, in_variant = FAMILIES[family]
    res = clean_record()
    res[kernels[0]] = {"vgprs": 32}
    expect = {"scan": [UNREAD_SCAN], "docs": [], "attention": [], "gemm": [UNREAD_GEMM],
              "batch": [FAMILIES["topic"][1], message]}.get(family, [message])   # (docs and attention: only a figure that is there refuses;
    #                                                                              kernels[0] of the batch is a topic kernel too)
    if variant and family == "refine":
        expect = []
    assert heads(build.refusals(res, variant)) == expect


def test_a_seventeenth_scan_kernel_without_figures_does_not_blind_the_check():
    res = clean_record()
    res["k_scan_extra"] = {}
    assert build.refusals(res) == []


def test_a_variant_build_lets_through_exactly_the_product_only_checks():
    """every product-only condition at once: a variant build passes, the product build names all of them in the table's order;
    and the conditions a variant shares are refused alike"""
    res = clean_record()
    res["k_refine"]["spill_vgprs"] = 3
    res["k_enc_attention_mfma"]["scratch_bytes"] = 16
    res["k_enc_gemm_0"]["scratch_bytes"] = 8
    assert build.refusals(res, variant=True) == []
    assert heads(build.refusals(res, variant=False)) == [FAMILIES["refine"][1], FAMILIES["attention"][1], FAMILIES["gemm"][1]]
    shared = copy.deepcopy(res)
    del shared["k_refine_spill"]                  # (refine a kernel short: still the product's business only)
    del shared["k_enc_gemm_5"]                    # (gemm a kernel short: refused in a variant too)
    shared["k_fuse_rrf"]["spill_vgprs"] = 1
    assert heads(build.refusals(shared, variant=True)) == [FAMILIES["fuse"][1],
                                                           "the compiler's resource remarks could not be read for the k_enc_gemm kernels (5 found)"]

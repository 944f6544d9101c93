"""The XLM-R forward over the packed real tokens of a batch (`_PackedEncoder`: what `EmbeddingProvider` and the cross-encoder reranker run),
split into plan_forward() — which path a batch takes, a pure function that tests/test_forward_plan.py pins as a table — and the code
that executes the plan; with it the hashing tokenizer and the architecture constants of the random-init models."""
from __future__ import annotations

import logging
import os
import zlib
from collections import namedtuple
from types import SimpleNamespace
from typing import List, NamedTuple, Optional

import numpy as np
import torch

logger = logging.getLogger(__name__)

# XLM-RoBERTa-large = BGE-M3's backbone (24 layers x 1024 hidden x 16 heads, FFN 4096, vocab 250 002)
_XLMR_LARGE = dict(vocab_size=250002, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
                   intermediate_size=4096, max_position_embeddings=8194, type_vocab_size=1, pad_token_id=1,
                   bos_token_id=0, eos_token_id=2, layer_norm_eps=1e-5)


class _HashTokenizer:
    """whitespace pieces -> crc32 ids; only for random-init benchmarking (no sentencepiece model offline). The id of a piece is
    remembered (a real tokenizer's vocabulary lookup is a hash-table hit too) and the padded batch is assembled in numpy: 1024
    short questions take ~1.5 ms instead of 10 — the encode leg of BASELINE config 5 measures the GPU, not this stand-in."""

    def __init__(self, vocab_size: int, max_len: int = 512):
        self.vocab_size, self.max_len = vocab_size, max_len
        self._ids: dict = {}

    def __call__(self, texts: List[str]):
        cap, n = self.max_len - 2, len(texts)
        toks = [t.split()[:cap] for t in texts]
        lens = np.fromiter(map(len, toks), dtype=np.int64, count=n)
        words = [w for tk in toks for w in tk]
        ids = self._piece_ids(words)
        width = int(lens.max()) + 2 if n else 2
        inp = np.full((n, width), 1, dtype=np.int64)       # <pad> = 1
        if n:
            inp[:, 0] = 0                                  # <s>
            first = np.cumsum(lens) - lens
            row = np.repeat(np.arange(n), lens)
            inp[row, np.arange(len(words)) - np.repeat(first, lens) + 1] = np.asarray(ids, dtype=np.int64)
            inp[np.arange(n), lens + 1] = 2                # </s>
        att = (np.arange(width)[None, :] < (lens + 2)[:, None]).astype(np.int64)
        return {"input_ids": torch.from_numpy(inp), "attention_mask": torch.from_numpy(att)}

    def _piece_ids(self, words: List[str]) -> List[int]:
        ids = list(map(self._ids.get, words))              # vocabulary lookup at C speed; misses (None) are hashed once
        if None in ids:
            for j, v in enumerate(ids):
                if v is None:
                    w = words[j]
                    v = 4 + zlib.crc32(w.encode("utf-8")) % (self.vocab_size - 4)
                    if len(self._ids) < 1_000_000:
                        self._ids[w] = v
                    ids[j] = v
        return ids

    def pairs(self, queries: List[str], texts: List[str], max_length: int):
        """(query, text) pairs as ONE sequence each, XLM-R's pair layout `<s> q </s></s> d </s>`, cut to max_length tokens
        longest-first (a token comes off the longer side, off the text on a tie: what the tokenizers library does)."""
        rows = []
        budget = max_length - 4
        for q, d in zip(queries, texts):
            a, b = q.split(), d.split()
            la, lb = len(a), len(b)
            if la + lb > budget:                         # closed form of "drop one from the longer side until it fits"
                short = min(la, lb)
                if short * 2 >= budget:
                    la, lb = (budget + 1) // 2, budget // 2
                elif la > lb:
                    la = budget - lb
                else:
                    lb = budget - la
            rows.append((a[:la], b[:lb]))
        n = len(rows)
        lens = np.fromiter((len(a) + len(b) + 4 for a, b in rows), dtype=np.int64, count=n)
        width = int(lens.max()) if n else 4
        inp = np.full((n, width), 1, dtype=np.int64)       # <pad> = 1
        for i, (a, b) in enumerate(rows):
            ids = self._piece_ids(a + b)
            inp[i, :lens[i]] = [0] + ids[:len(a)] + [2, 2] + ids[len(a):] + [2]
        att = (np.arange(width)[None, :] < lens[:, None]).astype(np.int64)
        return {"input_ids": torch.from_numpy(inp), "attention_mask": torch.from_numpy(att)}


def _resolve_local_dir(model_name: str, cache_dir: Optional[str]) -> Optional[str]:
    cands = [model_name]
    if cache_dir:
        cands += [os.path.join(cache_dir, model_name), os.path.join(cache_dir, model_name.replace("/", "_")),
                  os.path.join(cache_dir, "models--" + model_name.replace("/", "--"))]
    for c in cands:
        if os.path.isdir(c):
            if os.path.exists(os.path.join(c, "config.json")):
                return c
            snaps = os.path.join(c, "snapshots")   # HF hub cache layout
            if os.path.isdir(snaps):
                for s in sorted(os.listdir(snaps)):
                    if os.path.exists(os.path.join(snaps, s, "config.json")):
                        return os.path.join(snaps, s)
    return None


class ForwardPlan(NamedTuple):
    """what one forward runs; `_PackedEncoder.cls()` computes it once and executes it"""
    layout: str              # "padded" (Q, K, V scattered into [batch][seq] around torch's SDPA) | "packed" (librdx kernels, nothing padded)
    projections: str         # "blas" | "small" (rdx_enc_linear_small_f16) | "stage" (rdx_enc_stage_f16 & co.) | "rdx" (rdx_enc_gemm_f16)
    attention: str           # "sdpa" | "valu" (rdx_enc_attention_f16) | "small" (the stage path's) | "mfma" (rdx_enc_attention_mfma_f16)
    graph: Optional[tuple]   # None, or the key of the HIP graph: ("small", Tp, lb) | ("large", B, Tp, lb) | (B, T, max_len, nqb)
    tokens: int              # the token count the forward runs on: Tp under a canonical shape, else T
    window: int              # the attention's LDS window: the 16 / 32 / 64 promise of a canonical shape, else the longest text
    work_units: int          # 0, or the entries of the MFMA kernel's query-block list that travels with the batch


def _window_promise(max_len: int) -> int:
    """the longest text rounded up to 16 / 32 / 64: a canonical shape's promise to the attention kernel (its LDS window)"""
    return 16 if max_len <= 16 else (32 if max_len <= 32 else 64)


def plan_forward(caps, knobs, B: int, T: int, max_len: int, blocks: int = 0) -> ForwardPlan:
    """The path of a batch of B texts, T real tokens, the longest of max_len tokens, `blocks` 64-query blocks (sum of ceil(len / 64)).
    caps: what the constructor established (fused, small_linear, small_stage, gemm_shapes); knobs: the settable attributes read below;
    an encoder is both. The granule of a small canonical shape follows the REAL token count; the projections follow the count the
    forward runs on, which under a canonical shape is the padded one."""
    k = knobs
    rdx = lambda n: bool(caps.fused and caps.gemm_shapes and k.gemm == "rdx" and n >= k.GEMM_MIN_TOKENS and n > k.SMALL_TOKENS)   # noqa: E731
    short = max_len <= k.FUSED_MAX_TOKENS
    if not (caps.fused and (short or k.long_attention)):
        return ForwardPlan("padded", "rdx" if rdx(T) else "blas", "sdpa", None, T, max_len, 0)
    # the corpus side (chunk texts of hundreds of tokens; and large question batches when MFMA_MIN_TOKENS says so): the MFMA kernel,
    # one work unit per 64 queries
    mfma = not short or bool(k.long_attention and T >= k.MFMA_MIN_TOKENS)
    if k.graphs and B <= k.SMALL_TEXTS and short:
        # (<= 32 tokens run the stage kernels: their cost follows the activation rows a workgroup stages, so the canonical shapes
        #  are 8, 16, 24 and 32 tokens — a typical 20-token question pays for 24 rows, not 32)
        g = 8 if (caps.small_stage and T <= k.STAGE_TOKENS) else k.SMALL_TOKEN_GRANULE
        n, window = -(-T // g) * g, _window_promise(max_len)
        graph, mfma, units = ("small", n, window), False, 0          # (no work-unit list rides in a small canonical shape)
    elif k.graphs and k.large_graphs and short and T >= k.LARGE_TOKEN_GRANULE:
        # (B + extra work units; `extra` moves with T inside one canonical shape, so the list is filled up to B + granule units)
        g = k.LARGE_TOKEN_GRANULE
        n, window, units = -(-T // g) * g, _window_promise(max_len), (B + g if mfma else 0)
        graph = ("large", B, n, window)
    else:
        n, window, units = T, max_len, (blocks if mfma else 0)
        graph = (B, T, max_len, units) if k.graphs is True else None   # (the longest text sizes the attention's LDS window: part of the shape)
    if caps.small_stage and n <= k.STAGE_TOKENS:
        return ForwardPlan("packed", "stage", "small", graph, n, window, units)
    # one question, a question's sub-queries: weight-streaming projections, GELU in the epilogue
    proj = "small" if (caps.small_linear and n <= k.SMALL_TOKENS) else ("rdx" if rdx(n) else "blas")
    return ForwardPlan("packed", proj, "mfma" if mfma else "valu", graph, n, window, units)


def _canonical_texts(first: np.ndarray, lens: np.ndarray, Tp: int):
    """tok_first / tok_len (int32 [Tp]) of a canonical shape: the real texts' tokens, then one-token dummy texts up to Tp"""
    T = int(lens.sum())
    tf, tl = np.empty(Tp, dtype=np.int32), np.empty(Tp, dtype=np.int32)
    tf[:T], tf[T:] = np.repeat(first, lens), np.arange(T, Tp)
    tl[:T], tl[T:] = np.repeat(lens, lens), 1
    return tf, tl


def canonical(ids_packed: np.ndarray, col: np.ndarray, first: np.ndarray, lens: np.ndarray, Tp: int, n_first: int, pad: int):
    """The forward's five index arrays for T = len(ids_packed) real tokens padded to Tp with one-token dummy texts (they attend to
    themselves; nobody reads their rows): token ids and position ids (int64 [Tp]), the texts' first tokens (int64 [n_first], zeros
    behind the real ones), tok_first and tok_len (int32 [Tp]). Tp = T and n_first = len(lens): the batch as it is."""
    T, B = len(ids_packed), len(lens)
    tok, pos, fst = np.empty(Tp, dtype=np.int64), np.empty(Tp, dtype=np.int64), np.zeros(n_first, dtype=np.int64)
    tok[:T], tok[T:] = ids_packed, pad
    pos[:T], pos[T:] = col + (pad + 1), pad + 1
    fst[:B] = first
    return (tok, pos, fst) + _canonical_texts(first, lens, Tp)


def pack_blob(arrays) -> np.ndarray:
    """the five arrays of canonical() in ONE uint8 buffer: tok | pos | first | tok_first | tok_len, 24 Tp + 8 n_first bytes"""
    return np.concatenate([a.view(np.uint8) for a in arrays])


def unpack_blob(blob, Tp: int, n_first: int):
    """pack_blob()'s inverse as views of `blob`: a numpy uint8 array, or a torch uint8 tensor (the static buffer of a graph)"""
    i64, i32 = (torch.int64, torch.int32) if isinstance(blob, torch.Tensor) else (np.int64, np.int32)
    o1, o2, o3, o4 = 8 * Tp, 16 * Tp, 16 * Tp + 8 * n_first, 20 * Tp + 8 * n_first
    return blob[:o1].view(i64), blob[o1:o2].view(i64), blob[o2:o3].view(i64), blob[o3:o4].view(i32), blob[o4:].view(i32)


_ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731  (an optional tensor argument of a librdx call)
_Layer = namedtuple("_Layer", "wqkv bqkv dense_o ln1 inter out ln2")   # (wqkv: the three projections are ONE GEMM on concatenated weights)


class _PackedEncoder:
    """The XLM-R forward over the REAL tokens only (PyTorch-ROCm plumbing, the checkpoint's own modules and weights).

    transformers pads a batch to its longest text and runs every token-wise operation — QKV / output / FFN projections, GELU,
    residual adds, LayerNorms: all but the attention itself — over the padding too (BASELINE config 5's 1024 questions: 28 672
    token slots for 20 649 tokens). Here the hidden states stay PACKED ([T_real][hidden]) through the whole stack; only around
    the attention are Q, K, V scattered into the padded [batch][seq] layout (index_copy) and the context gathered back
    (index_select). The three projections are ONE GEMM on concatenated weights. About half the launches of the module-by-module
    forward (the encode of a batch is launch-bound on a busy host) and 28 % fewer GEMM rows for that batch. Same arithmetic per
    token as `XLMRobertaModel.forward` (post-LayerNorm blocks, erf GELU, position ids = padding_idx + 1 + index in the text,
    attention over the text's own tokens only): tests/test_embedding_provider.py compares the two. With `fused` (fp16 on a GPU)
    the attention and the add + LayerNorm pairs are librdx kernels working on the packed layout directly: nothing is ever padded."""

    def __init__(self, model, fused: bool = False, graphs="auto"):
        e = model.embeddings
        self.word, self.pos, self.typ, self.ln, self.pad = e.word_embeddings, e.position_embeddings, e.token_type_embeddings, e.LayerNorm, int(e.padding_idx)
        cfg = model.config
        if getattr(cfg, "hidden_act", "gelu") != "gelu" or getattr(cfg, "position_embedding_type", None) not in (None, "absolute"):
            raise ValueError("packed forward: unsupported configuration")
        self.heads, self.hidden, self.graphs = int(cfg.num_attention_heads), int(cfg.hidden_size), graphs
        self.layers = []
        for L in model.encoder.layer:
            a = L.attention
            wqkv = torch.cat([a.self.query.weight, a.self.key.weight, a.self.value.weight], 0).contiguous()
            bqkv = torch.cat([a.self.query.bias, a.self.key.bias, a.self.value.bias], 0).contiguous()
            self.layers.append(_Layer(wqkv, bqkv, a.output.dense, a.output.LayerNorm, L.intermediate.dense, L.output.dense, L.output.LayerNorm))
        self._pad_buf, self._graph, self._seen = {}, {}, {}   # the padded layout's QKV scratch by shape; graphs by key; sightings of a key
        # librdx's two encoder kernels (include/rdx.h: rdx_enc_attention_f16, rdx_enc_add_layernorm_f16) take the place of the
        # scatter -> padded attention -> transposing copy -> gather chain and of the add + LayerNorm pairs: fp16 on a GPU, 64-wide
        # heads, hidden a multiple of 512 up to 2048, texts up to FUSED_MAX_TOKENS tokens (the attention kernel is written for
        # questions: its work per token grows with the text). Anything else runs the torch operations of the padded layout.
        self._lib = None
        self.fused = self.small_linear = self.small_stage = self.gemm_shapes = False
        p0 = self.layers[0].wqkv
        if fused and p0.is_cuda and p0.dtype == torch.float16 and self.hidden // self.heads == 64 and self.hidden % 512 == 0 and self.hidden <= 2048:
            from . import _lib
            self._lib = _lib.load()          # raises RdxUnavailable: a GPU provider asked for its kernels and the library is missing
            self._last_error = _lib.last_error
            self.fused = True
            ffn = self.layers[0].inter.weight.shape[0]
            self.small_linear = self.hidden % 512 == 0 and ffn % 512 == 0   # (rdx_enc_linear_small_f16: inputs a multiple of 512 wide)
            # the five-launches-per-layer forward of one question (rdx_enc_stage_f16 & co., csrc/enc_small.hpp)
            self.small_stage = self.hidden in (512, 1024) and ffn in (512, 1024, 2048, 4096)
            self.gemm_shapes = ffn % 64 == 0   # (rdx_enc_gemm_f16: feature counts a multiple of 64; hidden is one of 512)
            self.stage_fpb_o = int(os.environ.get("RDX_ENC_FPB_O", self.STAGE_FPB_O))
            self.stage_fpb_f2 = int(os.environ.get("RDX_ENC_FPB_F2", self.STAGE_FPB_F2))

    def release(self):
        """gives the device memory back: the graphs first (their pools go back to the allocator), then the scratch, then the weights"""
        self._graph.clear()
        self._pad_buf.clear()
        self.layers = []

    # Question batches (every text <= FUSED_MAX_TOKENS) of at least this many tokens would take the MFMA attention kernel too. Alone it
    # wins (1024 questions: 39 us per layer against the VALU kernel's 57, profiles/r04/attention_mfma_bench.txt); inside config 5's
    # pipeline it LOSES: the encode of batch i+1 runs beside the MFMA-bound search of batch i, and a kernel on the vector ALU fills what
    # the scan leaves idle while a second MFMA kernel queues for the same pipes (encode 16.1 / 16.0 against 15.4 / 15.4 ms, step 31.96 /
    # 31.76 against 31.15 / 31.24 ms, profiles/r04/c5_n1_bench.json, c5_mfma_attention_for_questions_n1_bench.json). Default: never; developer knob RDX_ENC_MFMA_MIN.
    MFMA_MIN_TOKENS = int(os.environ.get("RDX_ENC_MFMA_MIN", str(1 << 40)))
    FUSED_MAX_TOKENS = 64       # up to here the VALU attention kernel (written for questions); beyond, the MFMA kernel (long_attention)
    long_attention = os.environ.get("RDX_ENC_LONG_ATTN", "mfma") != "torch"   # developer: "torch" = scatter -> SDPA -> gather for texts beyond 64 tokens

    # gemm = "rdx": the projections of a batch of at least GEMM_MIN_TOKENS tokens are librdx's MFMA GEMM with the epilogue fused in
    # (rdx_enc_gemm_f16, csrc/enc_gemm.hpp: QKV + bias, O + residual, FFN-up + GELU, FFN-down + residual) and the add + LayerNorm pairs
    # shrink to rdx_enc_layernorm_f16: no torch GEMM, GELU or add on the stream. Default "blas"; developer knob RDX_ENC_GEMM.
    # GEMM_MIN_TOKENS: the per-layer A/B of tools/enc_gemm_bench.py (profiles/enc_gemm/layer_ab.txt) found NO token count
    # from 257 to 30 720 at which the fused layer is not slower than the BLAS path (new / parent 1.14 - 1.35), so the constant keeps a value
    # that never triggers: gemm="rdx" runs the kernel only where the developer knob RDX_ENC_GEMM_MIN lowers it.
    gemm = os.environ.get("RDX_ENC_GEMM", "blas")
    GEMM_MIN_TOKENS = int(os.environ.get("RDX_ENC_GEMM_MIN", str(1 << 40)))

    # up to here the projections are librdx's weight-streaming kernel (rdx_enc_linear_small_f16) instead of the BLAS library's GEMM. Measured
    # (tools/enc_small_sweep.py, graph replay, XLM-R-large): one question (32 padded tokens) 1.71 -> 1.36 ms; at 64 tokens the two are
    # equal (1.74), beyond the kernel loses (every 16-feature workgroup re-reads all activations: 128 tokens 2.12 against 1.78 ms)
    SMALL_TOKENS = 32

    # HIP-graph replay of the fused forward: captured per shape the second time the shape is seen, replayed with ONE launch; the five
    # small index tensors go into static device buffers first. graphs = "auto" (default): batches of at most SMALL_TEXTS texts — the
    # reference's online path: embed_query(), or the <= 4 sub-queries of one question embedded together (rag_dpo_amd/retriever.py) —
    # whose ~200 tiny kernels are pure launch latency (measured, one question on XLM-R-large fp16: module forward 6.3 ms, this
    # forward eager 3.4, replayed 1.55). Such a batch is padded to a CANONICAL shape so that the graphs are few and always hit: real
    # tokens up to a multiple of SMALL_TOKEN_GRANULE with one-token dummy texts (they attend to themselves; nobody reads their rows),
    # the CLS index list up to SMALL_TEXTS entries, the longest text up to 16 / 32 / 64 (it sizes the attention's LDS window): at
    # most 24 shapes. Its five index arrays travel in ONE buffer: one pinned copy per question instead of five (each small copy is
    # ~15 us of stream time: 0.07 of a 0.95 ms embed_query). True: additionally every larger batch by its exact (texts, tokens,
    # longest text) shape (a batch of 1024 gains nothing on the GPU, 3 ms of host time; production batches rarely repeat a token
    # count). False: never. At most MAX_GRAPHS shapes are kept (least recently used out).
    graphs = "auto"
    # canonical-shape graphs for large question batches too (BASELINE config 5: 1024 texts, ~20 K tokens): its ~230 launches cost a busy
    # host 15 - 35 ms per encode (measured) against 15 ms of GPU time. Canonical shape = real tokens padded to a multiple
    # of LARGE_TOKEN_GRANULE with one-token dummy texts (<= 5 % more rows at 20 K tokens; nobody reads their outputs), the longest text
    # rounded to 16 / 32 / 64: consecutive batches of a serving loop hit the same graph, ONE launch per encode.
    large_graphs = os.environ.get("RDX_ENC_LARGE_GRAPHS", "1") != "0"
    LARGE_TOKEN_GRANULE = 1024
    MAX_LARGE_GRAPHS = 3
    MAX_GRAPHS = 64
    SMALL_TEXTS = 8
    SMALL_TOKEN_GRANULE = 32

    # One question (at most STAGE_TOKENS packed tokens, padded to 16 or 32): five launches per layer, csrc/enc_small.hpp. The output
    # projection and FFN-down have 1024 features: with 16 per workgroup they would occupy 64 CUs, so their workgroups take 8 / 4 rows of
    # the MFMA tile (developer knobs RDX_ENC_FPB_O / RDX_ENC_FPB_F2; measured values in DESIGN.md §10).
    STAGE_TOKENS = 32
    STAGE_FPB_O = 8
    STAGE_FPB_F2 = 8

    def _call(self, name: str, dev: torch.device, *args):
        """librdx's `name`(device index, *args, the current stream of dev); a non-zero return raises with the library's message"""
        if getattr(self._lib, name)(dev.index or 0, *args, torch.cuda.current_stream(dev).cuda_stream):
            raise RuntimeError(name + ": " + self._last_error())

    def _gemm(self, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, epi: int = 0, res: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out = epi(x w^T + b): 0 plain, 1 erf GELU, 2 res + half(x w^T + b) — rdx_enc_gemm_f16"""
        out = torch.empty((x.shape[0], w.shape[0]), dtype=x.dtype, device=x.device)
        self._call("rdx_enc_gemm_f16", x.device, x.data_ptr(), w.data_ptr(), b.data_ptr(), _ptr(res), x.shape[0], w.shape[0], w.shape[1], epi, out.data_ptr())
        return out

    def _ln(self, s: torch.Tensor, ln) -> torch.Tensor:
        out = torch.empty_like(s)
        self._call("rdx_enc_layernorm_f16", s.device, s.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), float(ln.eps), s.shape[0], s.shape[1], out.data_ptr())
        return out

    def _add_ln(self, a: torch.Tensor, b: torch.Tensor, ln) -> torch.Tensor:
        out = torch.empty_like(a)
        self._call("rdx_enc_add_layernorm_f16", a.device, a.data_ptr(), b.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), float(ln.eps),
                   a.shape[0], a.shape[1], out.data_ptr())
        return out

    # The FFN's erf GELU is the framework's operation (bit-equal to the module forward). librdx's in-place kernel (E13, rdx_enc_gelu_f16: the
    # same values to within one fp16 ulp) is 81 against 101 us behind a 148 us FFN1 GEMM at 20 K tokens, and NOTHING in the pipeline: c5
    # encode 15.71 / 15.73 against 15.87 / 15.80 ms, ingest 3 429 against 3 435 chunks/s (profiles/r04/gelu_inplace_ab.txt) — opt-in only.
    inplace_gelu = os.environ.get("RDX_ENC_GELU", "torch") == "inplace"

    def _gelu(self, x: torch.Tensor) -> torch.Tensor:
        """erf GELU of the FFN's first projection: the framework's, or (RDX_ENC_GELU=inplace) librdx's in-place kernel E13"""
        if not self.inplace_gelu or x.numel() % 8 or not x.is_contiguous():
            return torch.nn.functional.gelu(x)
        self._call("rdx_enc_gelu_f16", x.device, x.data_ptr(), x.numel())
        return x

    def _linear(self, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, gelu: bool = False) -> torch.Tensor:
        out = torch.empty((x.shape[0], w.shape[0]), dtype=x.dtype, device=x.device)
        self._call("rdx_enc_linear_small_f16", x.device, x.data_ptr(), w.data_ptr(), b.data_ptr(), x.shape[0], w.shape[0], w.shape[1], 1 if gelu else 0, out.data_ptr())
        return out

    def _attention(self, qkv: torch.Tensor, tok_first: torch.Tensor, tok_len: torch.Tensor, max_len: int, qb=None) -> torch.Tensor:
        T, hd = qkv.shape[0], self.hidden // self.heads
        ctx = torch.empty((T, self.hidden), dtype=qkv.dtype, device=qkv.device)
        if qb is not None:                # texts beyond FUSED_MAX_TOKENS (the corpus side): the flash-style MFMA kernel over 64-query blocks
            self._call("rdx_enc_attention_mfma_f16", qkv.device, qkv.data_ptr(), qb.data_ptr(), int(qb.shape[0]), self.heads, hd, hd ** -0.5, ctx.data_ptr())
        else:
            self._call("rdx_enc_attention_f16", qkv.device, qkv.data_ptr(), tok_first.data_ptr(), tok_len.data_ptr(), T, self.heads, hd, hd ** -0.5, int(max_len), ctx.data_ptr())
        return ctx

    def _stage(self, x, w, b, T, ln=None, y_out=None, res=None, rows=None, epi=0, fpb=0):
        out = torch.empty((T, w.shape[0]), dtype=torch.float16, device=w.device)
        ln_w, ln_b, eps = (ln.weight, ln.bias, float(ln.eps)) if ln is not None else (None, None, 0.0)
        self._call("rdx_enc_stage_f16", w.device, x.data_ptr(), _ptr(rows), _ptr(ln_w), _ptr(ln_b), eps, _ptr(y_out), w.data_ptr(), b.data_ptr(),
                   _ptr(res), T, w.shape[0], w.shape[1], epi, fpb, out.data_ptr())
        return out

    def _small_forward(self, tok, pos, first_d, tok_first) -> torch.Tensor:
        """[T <= 32] ids / positions -> fp32 [len(first_d)][hidden] CLS rows; librdx kernels only (no torch operation on the stream).
        Every stage carries the LayerNorm in front of it, so the layer's skeleton differs from _layers()'."""
        dev = tok.device
        T, H, n_cls = int(tok.shape[0]), self.hidden, int(first_d.shape[0])
        f16 = dict(dtype=torch.float16, device=dev)
        s = torch.empty((T, H), **f16)
        self._call("rdx_enc_embed_f16", dev, tok.data_ptr(), pos.data_ptr(), self.word.weight.data_ptr(), self.pos.weight.data_ptr(),
                   self.typ.weight.data_ptr(), T, H, s.data_ptr())
        ln, last = self.ln, len(self.layers) - 1
        for li, L in enumerate(self.layers):
            y = torch.empty((T, H), **f16)
            qkv = self._stage(s, L.wqkv, L.bqkv, T, ln=ln, y_out=y, epi=0)
            ctx = torch.empty((T, H), **f16)
            self._call("rdx_enc_attention_small_f16", dev, qkv.data_ptr(), tok_first.data_ptr(), T, self.heads, H // self.heads, (H // self.heads) ** -0.5, ctx.data_ptr())
            rows = None
            if li == last:                                   # everything behind the last attention is row-wise: only the CLS rows are needed
                rows, T = first_d, n_cls
            s1 = self._stage(ctx, L.dense_o.weight, L.dense_o.bias, T, res=y, rows=rows, epi=2, fpb=self.stage_fpb_o)
            y1 = torch.empty((T, H), **f16)
            f = self._stage(s1, L.inter.weight, L.inter.bias, T, ln=L.ln1, y_out=y1, epi=1)
            s = self._stage(f, L.out.weight, L.out.bias, T, res=y1, epi=2, fpb=self.stage_fpb_f2)
            ln = L.ln2
        o = torch.empty((n_cls, H), dtype=torch.float32, device=dev)
        self._call("rdx_enc_layernorm_rows_f16", dev, s.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), float(ln.eps), n_cls, H, o.data_ptr())
        return o

    def _layer_ops(self, plan: ForwardPlan):
        """-> qkv(x, L), attn_out(ctx, x, L), ffn(x, L): who runs the token-wise steps of layer L under this plan"""
        F, g, ln, lin, add_ln, gelu = torch.nn.functional, self._gemm, self._ln, self._linear, self._add_ln, self._gelu
        if plan.projections == "rdx":
            # librdx's GEMM with fused epilogues: QKV + bias, O + residual, LayerNorm, FFN-up + GELU, FFN-down + residual, LayerNorm
            return (lambda x, L: g(x.contiguous(), L.wqkv, L.bqkv),
                    lambda ctx, x, L: ln(g(ctx, L.dense_o.weight, L.dense_o.bias, 2, x.contiguous()), L.ln1),
                    lambda x, L: ln(g(g(x, L.inter.weight, L.inter.bias, 1), L.out.weight, L.out.bias, 2, x), L.ln2))
        if plan.projections == "small":
            return (lambda x, L: lin(x, L.wqkv, L.bqkv),
                    lambda ctx, x, L: add_ln(lin(ctx, L.dense_o.weight, L.dense_o.bias), x, L.ln1),
                    lambda x, L: add_ln(lin(lin(x, L.inter.weight, L.inter.bias, gelu=True), L.out.weight, L.out.bias), x, L.ln2))
        if plan.layout == "packed":
            return (lambda x, L: F.linear(x, L.wqkv, L.bqkv),
                    lambda ctx, x, L: add_ln(L.dense_o(ctx), x, L.ln1),
                    lambda x, L: add_ln(L.out(gelu(L.inter(x))), x, L.ln2))
        return (lambda x, L: F.linear(x, L.wqkv, L.bqkv),
                lambda ctx, x, L: L.ln1(L.dense_o(ctx) + x),
                lambda x, L: L.ln2(L.out(F.gelu(L.inter(x))) + x))

    def _layers(self, plan: ForwardPlan, x, first_d, attend) -> torch.Tensor:
        """every layer over the embeddings x [T][H]: QKV projection -> attend(qkv) -> O-projection + residual + LN -> FFN + residual + LN"""
        qkv, attn_out, ffn = self._layer_ops(plan)
        last = len(self.layers) - 1
        for li, L in enumerate(self.layers):
            ctx = attend(qkv(x, L))                                                                                # [T][H]
            if li == last:                                   # everything behind the last attention is row-wise: only the CLS rows are needed
                ctx, x = ctx.index_select(0, first_d), x.index_select(0, first_d)
            x = ffn(attn_out(ctx, x, L), L)
        return x.to(torch.float32)

    def _fused_forward(self, plan: ForwardPlan, tok, pos, first_d, tok_first, tok_len, qb=None) -> torch.Tensor:
        """the forward on packed tokens with librdx's kernels: [T] ids / positions -> fp32 [B][hidden] CLS rows, no padding anywhere"""
        if plan.projections == "stage":
            return self._small_forward(tok, pos, first_d, tok_first)
        qb = qb if plan.attention == "mfma" else None
        x = self.ln(self.word(tok) + self.pos(pos) + self.typ.weight[0])                                         # [T][H]
        return self._layers(plan, x, first_d, lambda qkv: self._attention(qkv, tok_first, tok_len, plan.window, qb))

    def _padded_forward(self, plan: ForwardPlan, ids_packed, row, col, first, lens, B: int, S: int, to_dev) -> torch.Tensor:
        """the forward with torch's attention: Q, K, V scattered into the padded [B][S] layout around it, the context gathered back"""
        F, H, nh = torch.nn.functional, self.hidden, self.heads
        tok, pos, first_d = to_dev("pk_tok", torch.from_numpy(ids_packed)), to_dev("pk_pos", torch.from_numpy(col + (self.pad + 1))), to_dev("pk_first", torch.from_numpy(first))
        x = self.ln(self.word(tok) + self.pos(pos) + self.typ.weight[0])                                         # [T][H]
        flat_d = to_dev("pk_flat", torch.from_numpy(row * S + col))                                              # slot of packed token t in the padded [B*S] layout
        kmask = to_dev("pk_mask", torch.from_numpy(np.arange(S)[None, :] < lens[:, None])).view(B, 1, 1, S)       # keys of the text itself
        key = (B, S, x.dtype, x.device)
        qkv_pad = self._pad_buf.get(key)
        if qkv_pad is None:
            if len(self._pad_buf) > 8:
                self._pad_buf.clear()
            qkv_pad = self._pad_buf[key] = torch.zeros((B * S, 3 * H), dtype=x.dtype, device=x.device)   # (stale padding slots are masked keys / dropped queries)

        def attend(qkv):
            qkv_pad.index_copy_(0, flat_d, qkv)
            q, k, v = qkv_pad.view(B, S, 3, nh, H // nh).permute(2, 0, 3, 1, 4)                                   # [B][heads][S][head_dim] views
            ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=kmask)
            return ctx.transpose(1, 2).reshape(B * S, H).index_select(0, flat_d)                                  # back to [T][H]
        return self._layers(plan, x, first_d, attend)

    _ORDER = ("pk_tok", "pk_pos", "pk_first", "pk_tfirst", "pk_tlen")

    def _replay(self, plan: ForwardPlan, host: dict, to_dev, unpack=None):
        """-> the CLS rows from a captured graph of this shape, or None (shape not captured: the caller runs eagerly).
        unpack: the forward's index tensors as views of the one static buffer host["pk_blob"] is copied into"""
        key = plan.graph
        args = (lambda st: unpack(st["pk_blob"])) if unpack is not None else (lambda st: tuple(st[n] for n in self._ORDER))
        if key[0] == "large" and key not in self._graph:
            big = [k_ for k_ in self._graph if k_[0] == "large"]
            if len(big) >= self.MAX_LARGE_GRAPHS:
                torch.cuda.current_stream(self.layers[0].wqkv.device).synchronize()   # (its last replay may still run)
                self._graph.pop(big[0])                           # each holds the activations of ~Tp tokens: keep few
        ent = self._graph.pop(key, None)
        if ent is None:
            if len(self._seen) > 4096:
                self._seen.clear()
            self._seen[key] = self._seen.get(key, 0) + 1
            if self._seen[key] < 2:
                return None
            while len(self._graph) >= self.MAX_GRAPHS:
                torch.cuda.current_stream(self.layers[0].wqkv.device).synchronize()   # (its last replay may still run: its pool is freed with it)
                self._graph.pop(next(iter(self._graph)))          # least recently used (dicts keep insertion order; a hit re-inserts)
            dev = self.layers[0].wqkv.device
            static = {n: torch.empty(tuple(t.shape), dtype=t.dtype, device=dev) for n, t in host.items()}
            for n, t in host.items():
                to_dev(n, t, static[n])
            try:
                side = torch.cuda.Stream(device=dev)             # one eager run on a side stream first (library workspaces), as torch asks
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    self._fused_forward(plan, *args(static), static.get("pk_qb"))
                torch.cuda.current_stream(dev).wait_stream(side)
                g = torch.cuda.CUDAGraph()
                # thread-local capture mode: only THIS thread's calls are restricted while the capture runs — a search another
                # thread has in flight on the same device (one shared provider and collection serve concurrent sessions, reference
                # app.py:42-43) may allocate and synchronise as it likes
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    out = self._fused_forward(plan, *args(static), static.get("pk_qb"))
            except Exception as e:                               # noqa: BLE001  (a capture that fails costs speed only: eager from now on)
                logger.warning(f"encoder graph capture failed ({e!r}); the forward stays eager")
                self.graphs = False
                return None
            ent = (g, static, out)
        self._graph[key] = ent
        g, static, out = ent
        for n, t in host.items():
            to_dev(n, t, static[n])
        g.replay()
        return out                                               # (overwritten by the next replay of this shape: consume it on the stream)

    @staticmethod
    def _query_blocks(first: np.ndarray, lens: np.ndarray) -> torch.Tensor:
        """The MFMA attention kernel's work units: one per 64 queries of a text, {first token, length, first query, 0}."""
        nb = (lens + 63) // 64
        tix = np.repeat(np.arange(len(lens), dtype=np.int64), nb)
        q0 = (np.arange(int(nb.sum()), dtype=np.int64) - np.repeat(np.cumsum(nb) - nb, nb)) * 64
        return torch.from_numpy(np.stack([first[tix], lens[tix], q0, np.zeros_like(q0)], axis=1).astype(np.int32))

    @classmethod
    def _canonical_query_blocks(cls, first: np.ndarray, lens: np.ndarray, Tp: int, units: int) -> torch.Tensor:
        """the MFMA kernel's work units of a canonical shape: the real texts' and the dummies', then repeats of the last unit up to
        `units` (the same rows written twice with the same values)"""
        T = int(lens.sum())
        qb = cls._query_blocks(np.concatenate([first, np.arange(T, Tp, dtype=np.int64)]), np.concatenate([lens, np.ones(Tp - T, dtype=np.int64)]))
        return torch.cat([qb, qb[-1:].expand(units - qb.shape[0], 4)]).contiguous()

    _window_promise = staticmethod(_window_promise)
    _canonical_texts = staticmethod(_canonical_texts)

    @torch.no_grad()
    def cls(self, ids: torch.Tensor, lens: np.ndarray, to_dev) -> torch.Tensor:
        """ids: [B][S] int64 on the host, right-padded; lens[b] = tokens of text b (>= 1). -> fp32 [B][hidden] CLS rows on the device.
        to_dev(name, host tensor[, out]) -> device tensor (the provider's pinned, non-blocking copies)."""
        B, S = int(ids.shape[0]), int(ids.shape[1])
        lens = np.asarray(lens, dtype=np.int64)
        T = int(lens.sum())
        first = np.cumsum(lens) - lens                                   # packed index of every text's first token (CLS)
        row = np.repeat(np.arange(B, dtype=np.int64), lens)
        col = np.arange(T, dtype=np.int64) - np.repeat(first, lens)
        ids_packed = np.ascontiguousarray(ids.numpy()[row, col])
        plan = plan_forward(self, self, B, T, int(lens.max()), int(((lens + 63) // 64).sum()))   # (an encoder is its own caps and knobs)
        if plan.layout == "padded":
            return self._padded_forward(plan, ids_packed, row, col, first, lens, B, S, to_dev)
        Tp, small = plan.tokens, plan.graph is not None and plan.graph[0] == "small"
        arrays = canonical(ids_packed, col, first, lens, Tp, self.SMALL_TEXTS if small else B, self.pad)
        if small:
            host, unpack = {"pk_blob": torch.from_numpy(pack_blob(arrays))}, (lambda d: unpack_blob(d, Tp, self.SMALL_TEXTS))
        else:
            host, unpack = dict(zip(self._ORDER, map(torch.from_numpy, arrays))), None
            if plan.work_units:
                host["pk_qb"] = self._canonical_query_blocks(first, lens, Tp, plan.work_units)
        out = self._replay(plan, host, to_dev, unpack) if plan.graph is not None else None
        if out is None:   # no graph (yet): the SAME padded tensors eagerly, so that call 1 and the replays run identical shapes
            dev = {n: to_dev(n, t) for n, t in host.items()}
            out = self._fused_forward(plan, *(unpack(dev["pk_blob"]) if small else (dev[n] for n in self._ORDER)), dev.get("pk_qb"))
        return out[:B] if small else out

    @torch.no_grad()
    def tokens(self, ids: torch.Tensor, lens: np.ndarray, to_dev) -> torch.Tensor:
        """cls()'s arguments -> fp32 [T][hidden] final hidden states of ALL packed tokens (text b's are rows first[b] .. first[b] +
        lens[b], <s> first): what BGE-M3's per-token (ColBERT) head reads. The eager packed forward with every row selected behind the
        last attention; no graph replay, no canonical shape, and not the one-question stage kernels (their last layer is written
        for the <s> rows). cls() and the plans it takes are untouched."""
        B, S = int(ids.shape[0]), int(ids.shape[1])
        lens = np.asarray(lens, dtype=np.int64)
        T = int(lens.sum())
        first = np.cumsum(lens) - lens
        row = np.repeat(np.arange(B, dtype=np.int64), lens)
        col = np.arange(T, dtype=np.int64) - np.repeat(first, lens)
        ids_packed = np.ascontiguousarray(ids.numpy()[row, col])
        every = np.arange(T, dtype=np.int64)
        caps = SimpleNamespace(fused=self.fused, small_linear=self.small_linear, small_stage=False, gemm_shapes=self.gemm_shapes)
        knobs = SimpleNamespace(graphs=False, **{k: getattr(self, k) for k in (
            "gemm", "GEMM_MIN_TOKENS", "SMALL_TOKENS", "FUSED_MAX_TOKENS", "long_attention", "MFMA_MIN_TOKENS", "SMALL_TEXTS", "STAGE_TOKENS",
            "SMALL_TOKEN_GRANULE", "large_graphs", "LARGE_TOKEN_GRANULE")})
        plan = plan_forward(caps, knobs, B, T, int(lens.max()), int(((lens + 63) // 64).sum()))
        if plan.layout == "padded":
            return self._padded_forward(plan, ids_packed, row, col, every, lens, B, S, to_dev)
        tok, pos, _, tok_first, tok_len = canonical(ids_packed, col, first, lens, T, B, self.pad)
        host = dict(zip(self._ORDER, map(torch.from_numpy, (tok, pos, every, tok_first, tok_len))))
        if plan.work_units:
            host["pk_qb"] = self._query_blocks(first, lens)
        dev = {n: to_dev(n, t) for n, t in host.items()}
        return self._fused_forward(plan, *(dev[n] for n in self._ORDER), dev.get("pk_qb"))

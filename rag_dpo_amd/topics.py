"""TopicMatcher — same interface as reference src/utils/rgpd_topics.py:134-222, MI355X backend.

Reference behaviour mirrored (file:line in the reference's src/utils/rgpd_topics.py):
  ctor embedding_provider (None: only exact matches boost)                                  :143-150
  _get_embedding(text): cached; None without a provider or when the embed raises (not cached)  :152-163
  similarity(a, b): the dot product of the two embeddings, 0.0 when either is missing         :165-176
  topic_boost(question_topics, chunk_tags_str, threshold=0.65): tags split on ',', stripped, empties dropped; best starts at 0.0,
      strict '>'; a case-insensitive exact match sets 1.0 and leaves the tag loop, best >= 1.0 leaves the topic loop;
      0.0 below the threshold, else 0.15 * (best - threshold) / (1.0 - threshold)              :178-222

What differs underneath. The reference embeds one string per `embed([tag])` and dots Python-float arrays per candidate. Here
  - `topic_boosts` / `topic_boosts_device` take ALL candidates of a question: the call's distinct strings that have no embedding yet go
    to the provider as one batch (`embed_device` when it has one, else `embed`; a batch that raises is retried string by string, so
    a bad tag costs that tag only and is tried again by the next call that meets it);
  - the embeddings live in one fp32 table [capacity][dim] on the matcher's device (it doubles when full), a dict maps text -> row;
  - on a GPU one `rdx_topic_boost` call (include/rdx.h) computes the similarities and replays the reference's loops for every
    candidate; the fp64 boosts stay on the device, where `rdx_rerank_select` reads them.
Arithmetic. Embeddings are kept in fp32 (what this project's providers return; a provider that hands out wider values has them
rounded once). A similarity is the fp64 sum of the exact products in the kernel's documented order (csrc/topic_kernel.hpp), on the GPU
and in the host evaluator below alike: the two agree bit for bit, and differ from numpy's `dot` of the reference by the order of the
additions only (|d sim| <= dim * 2^-53 * sum |a_i b_i|). `embed_device` of this project's provider returns rows that are NOT yet
normalised; they are normalised here by `rdx_l2_normalize`, the very step `embed()` applies, so both ways store the same bits.
A call beyond the kernel's limits (1024 candidates, 32 topics, 64 tags per candidate, dim 4096) is evaluated by the host evaluator.
`topic_boosts_device_batch` does the same for the candidates of SEVERAL questions: one `_Plan` per question, one embed call for the
batch's unseen strings, one upload and one `rdx_topic_boost_batch` call; per question the bits of
`topic_boosts_device`."""
from __future__ import annotations

import logging
import threading
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

logger = logging.getLogger(__name__)

MAX_BOOST = 0.15                 # rgpd_topics.py:220
DEFAULT_THRESHOLD = 0.65         # rgpd_topics.py:182


def split_tags(chunk_tags_str) -> List[str]:
    """rgpd_topics.py:195-198"""
    if not chunk_tags_str:
        return []
    return [t.strip() for t in chunk_tags_str.split(',') if t.strip()]


def dots_kernel_order(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp64 [T][U] dot products of the fp32 rows a [T][dim] and b [U][dim] in rdx_topic_boost's order: 64 partial sums (partial l adds
    the products of elements l, l + 64, ... one after the other, from +0.0), then s[l] += s[l ^ m] for m = 32, ..., 1"""
    a64, b64 = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    T, U, dim = a64.shape[0], b64.shape[0], a64.shape[1]
    acc = np.zeros((T, U, 64), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, dim, 64):
            w = min(64, dim - i0)
            acc[:, :, :w] += a64[:, None, i0:i0 + w] * b64[None, :, i0:i0 + w]     # (the products are exact: one rounding, the add's)
        lanes = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, :, lanes ^ m]
    return acc[:, :, 0]


class _Plan:
    """one call's inputs of rdx_topic_boost, as host lists: the topics' and the distinct tags' strings, and per candidate the
    (topic index, tag index, exact) pairs in the reference's loop order (cut behind an exact pair: the replay ends there)"""
    __slots__ = ("topics", "tags", "offsets", "pairs", "max_tags")

    def __init__(self, question_topics: Sequence[str], chunk_tags_strs: Sequence):
        self.topics = list(question_topics) if question_topics else []
        self.tags: List[str] = []
        index: Dict[str, int] = {}
        self.offsets = [0]
        self.pairs: list = []
        self.max_tags = 0
        lowered = [t.lower() for t in self.topics]
        per_string: Dict[str, list] = {}
        for s in chunk_tags_strs:
            words = per_string.get(s) if isinstance(s, str) else None
            if words is None:
                words = []
                tags = split_tags(s) if self.topics else []
                self.max_tags = max(self.max_tags, len(tags))
                ids = []
                for t in tags:
                    u = index.get(t)
                    if u is None:
                        u = index[t] = len(self.tags)
                        self.tags.append(t)
                    ids.append(u)
                low = [t.lower() for t in tags]
                done = False
                for ti, tl in enumerate(lowered):
                    for u, l in zip(ids, low):
                        exact = tl == l
                        words.append((ti, u, exact))
                        if exact:
                            done = True
                            break
                    if done:
                        break
                if isinstance(s, str):
                    per_string[s] = words
            self.pairs.extend(words)
            self.offsets.append(len(self.pairs))

    def strings(self) -> List[str]:
        return list(dict.fromkeys(self.topics + self.tags)) if self.tags else []


def pack_plans(plans: Sequence[_Plan], slot_of) -> dict:
    """The plans of several questions in rdx_topic_boost_batch's layout (include/rdx.h), as host arrays. Question q's topics are
    topic_slots[topic_off[q]:topic_off[q + 1]], its distinct tags tag_slots[tag_off[q]:tag_off[q + 1]], its candidates the segment
    [cand_off[q], cand_off[q + 1]) of the candidate axis and its similarity block starts at sim_off[q] ([T_q][U_q] doubles, one
    block behind the other). pair_off (int64) is ONE running offset array over the whole axis; the pair words keep the topic and tag
    indices LOCAL to their question, exactly the words a single-question call gets. slot_of: text -> table row, or -1."""
    from . import _lib as L
    nq = len(plans)
    topic_off, tag_off, cand_off = (np.zeros((nq + 1,), dtype=np.int32) for _ in range(3))
    sim_off = np.zeros((nq + 1,), dtype=np.int64)
    topic_slots, tag_slots, pair_off, pairs = [], [], [0], []
    for q, plan in enumerate(plans):
        T, U, n = len(plan.topics), len(plan.tags), len(plan.offsets) - 1
        topic_slots.extend(slot_of(t) for t in plan.topics)
        tag_slots.extend(slot_of(t) for t in plan.tags)
        base = len(pairs)
        pairs.extend(L.topic_pair(t, u, e) for t, u, e in plan.pairs)
        pair_off.extend(base + o for o in plan.offsets[1:])
        topic_off[q + 1], tag_off[q + 1], cand_off[q + 1] = topic_off[q] + T, tag_off[q] + U, cand_off[q] + n
        sim_off[q + 1] = sim_off[q] + T * U
    return {"topic_off": topic_off, "tag_off": tag_off, "cand_off": cand_off, "sim_off": sim_off,
            "topic_slots": np.asarray(topic_slots, dtype=np.int32), "tag_slots": np.asarray(tag_slots, dtype=np.int32),
            "pair_off": np.asarray(pair_off, dtype=np.int64), "pairs": np.asarray(pairs, dtype=np.int32)}


class _PinnedRing:
    """Four pinned int32 host buffers used in turn. A slot is [buffer, event]: the event stands behind the last device work that
    reads the buffer and is waited on before the buffer is written again; a buffer too small for a call is replaced by one of
    twice the call's words."""
    SLOTS = 4

    def __init__(self, min_words: int):
        self.min_words = min_words
        self.slots: list = []
        self.next = 0

    def put(self, words: np.ndarray):
        """int32 host words -> (the pinned tensor holding them, its slot); the caller records slot[1] behind what reads the tensor"""
        if len(self.slots) < self.SLOTS:
            self.slots.append([torch.empty((max(self.min_words, 2 * len(words)),), dtype=torch.int32).pin_memory(), None])
            slot = self.slots[-1]
        else:
            slot = self.slots[self.next]
            self.next = (self.next + 1) % len(self.slots)
            if slot[1] is not None:
                slot[1].synchronize()
            if slot[0].numel() < len(words):
                slot[0] = torch.empty((2 * len(words),), dtype=torch.int32).pin_memory()
        buf = slot[0][:len(words)]
        buf.numpy()[:] = words
        return buf, slot


class TopicMatcher:
    """Semantic matching of question topics and chunk tags; one instance serves every session, as the provider does."""

    GROW_FROM = 256              # rows of the first table
    WARM_BATCH = 256             # strings per embed call of warm()

    def __init__(self, embedding_provider=None, device=None):
        self._embedder = embedding_provider
        if device is None:
            device = getattr(embedding_provider, "device", "cpu") if embedding_provider is not None else "cpu"
            if str(device).startswith("cuda") and not torch.cuda.is_available():
                device = "cpu"
        self.device = torch.device(str(device))
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.on_gpu = self.device.type == "cuda"
        self._lock = threading.RLock()
        self._slots: Dict[str, int] = {}
        self._table = None           # fp32 [capacity][dim]: a device tensor on a GPU, a numpy array on the CPU
        self._dim: Optional[int] = None
        self._lib = None
        self._staging = _PinnedRing(4096)   # the plans' uploads: a slot's event stands behind the copy that read it
        self._shapes = _PinnedRing(1024)    # the batched calls' shape arrays: a slot's event stands behind the kernels that read it
        self.stats = {"embed_calls": 0, "embedded": 0, "device_calls": 0, "host_calls": 0}
        if self.on_gpu:
            from . import _lib
            self._lib = _lib.load()              # raises RdxUnavailable: the GPU path has no torch substitute

    # ---- the tag table -------------------------------------------------------------------------------------------------------
    @property
    def size(self) -> int:
        """strings that have an embedding in the table"""
        return len(self._slots)

    @property
    def capacity(self) -> int:
        return 0 if self._table is None else int(self._table.shape[0])

    def _embed_rows(self, texts: List[str]):
        """one provider call -> fp32 [len(texts)][dim] unit rows where the table lives"""
        self.stats["embed_calls"] += 1
        e = self._embedder
        if self.on_gpu and hasattr(e, "embed_device"):
            raw = e.embed_device(list(texts))
            if not isinstance(raw, torch.Tensor) or raw.dim() != 2 or raw.shape[0] != len(texts):
                raise ValueError("embed_device did not return one row per text")
            raw = raw.to(device=self.device, dtype=torch.float32).contiguous()
            from . import _lib as L
            out = torch.empty_like(raw)
            L.check(self._lib.rdx_l2_normalize(self.device.index, raw.data_ptr(), raw.shape[0], raw.shape[1], out.data_ptr(), L.RDX_DEVICE,
                                               torch.cuda.current_stream(self.device).cuda_stream))
            return out
        vecs = e.embed(list(texts))
        if len(vecs) != len(texts):
            raise ValueError("embed did not return one vector per text")
        with np.errstate(over="ignore"):
            rows = np.ascontiguousarray(np.asarray(vecs, dtype=np.float32))
        if rows.ndim != 2:
            raise ValueError("embed did not return vectors of one length")
        return torch.from_numpy(rows).to(self.device) if self.on_gpu else rows

    def _store(self, texts: List[str], rows) -> None:
        """(under the lock) appends the rows; the slots are published once the rows are in place"""
        m, dim = int(rows.shape[0]), int(rows.shape[1])
        if self._dim is None:
            self._dim = dim
        if dim != self._dim:
            raise ValueError(f"TopicMatcher: the provider returned {dim}-dimensional embeddings, the table holds {self._dim}")
        count = len(self._slots)
        if self._table is None or count + m > self.capacity:
            cap = max(self.GROW_FROM, self.capacity)
            while cap < count + m:
                cap *= 2
            if self.on_gpu:
                new = torch.empty((cap, dim), dtype=torch.float32, device=self.device)
                if count:
                    new[:count] = self._table[:count]
                torch.cuda.synchronize(self.device)      # a call of another session may still read the old table: it is dropped below
            else:
                new = np.empty((cap, dim), dtype=np.float32)
                if count:
                    new[:count] = self._table[:count]
            self._table = new
        self._table[count:count + m] = rows
        if self.on_gpu:
            torch.cuda.current_stream(self.device).synchronize()   # sessions on other streams read a slot as soon as the dict has it
        for i, t in enumerate(texts):
            self._slots[t] = count + i
        self.stats["embedded"] += m

    def _ensure(self, texts: Sequence[str]) -> None:
        """embeds the distinct strings that have no slot yet, in one batch; a batch that raises is retried string by string"""
        if self._embedder is None:
            return
        with self._lock:
            missing = [t for t in dict.fromkeys(texts) if t not in self._slots]
            if not missing:
                return
            try:
                self._store(missing, self._embed_rows(missing))
                return
            except Exception as e:  # noqa: BLE001
                if len(missing) == 1:
                    logger.debug(f"Embedding tag '{missing[0]}' failed: {e}")
                    return
                logger.debug(f"embedding a batch of {len(missing)} tags failed ({e}): retrying one by one")
            for t in missing:
                try:
                    self._store([t], self._embed_rows([t]))
                except Exception as e:  # noqa: BLE001  (rgpd_topics.py:160-162: no embedding, nothing cached)
                    logger.debug(f"Embedding tag '{t}' failed: {e}")

    def warm(self, texts: Sequence[str]) -> int:
        """embeds the distinct strings ahead of time, WARM_BATCH per provider call -> how many were new"""
        before = len(self._slots)
        todo = [t for t in dict.fromkeys(texts) if t and t not in self._slots]
        for a in range(0, len(todo), self.WARM_BATCH):
            self._ensure(todo[a:a + self.WARM_BATCH])
        return len(self._slots) - before

    def warm_from_collection(self, collection, key: str = "rgpd_topics", page: int = 5000) -> int:
        """warm() over the distinct tags of a collection's metadata, read in pages of `page` rows"""
        tags: Dict[str, None] = {}
        offset = 0
        while True:
            got = collection.get(limit=page, offset=offset, include=["metadatas"])
            metas = got.get("metadatas") or []
            for m in metas:
                for t in split_tags((m or {}).get(key, "")):
                    tags[t] = None
            if len(got.get("ids") or metas) < page:
                break
            offset += page
        return self.warm(list(tags))

    def _rows_host(self, slots: Sequence[int]) -> np.ndarray:
        """fp32 host copies of table rows (slot -1: zeros, never used)"""
        idx = np.asarray(slots, dtype=np.int64)
        if self._table is None:
            return np.zeros((len(idx), 1), dtype=np.float32)
        safe = np.where(idx >= 0, idx, 0)
        if self.on_gpu:
            return self._table[torch.from_numpy(safe).to(self.device)].cpu().numpy()
        return self._table[safe]

    # ---- the reference's methods -----------------------------------------------------------------------------------------------
    def _get_embedding(self, text: str) -> Optional[np.ndarray]:
        if self._embedder is None:
            return None
        self._ensure([text])
        with self._lock:
            slot = self._slots.get(text)
            return None if slot is None else self._rows_host([slot])[0].copy()

    def similarity(self, tag_a: str, tag_b: str) -> float:
        vec_a = self._get_embedding(tag_a)
        vec_b = self._get_embedding(tag_b)
        if vec_a is None or vec_b is None:
            return 0.0
        return float(dots_kernel_order(vec_a[None, :], vec_b[None, :])[0, 0])

    def topic_boost(self, question_topics: List[str], chunk_tags_str: str, threshold: float = DEFAULT_THRESHOLD) -> float:
        return self.topic_boosts(question_topics, [chunk_tags_str], threshold)[0]

    # ---- all candidates of a question ------------------------------------------------------------------------------------------
    def topic_boosts(self, question_topics: List[str], chunk_tags_strs: Sequence[str], threshold: float = DEFAULT_THRESHOLD) -> List[float]:
        plan = self._plan(question_topics, chunk_tags_strs)
        if self._fits_kernel(plan, threshold):
            return self._device(plan, threshold).cpu().tolist()
        return self._host(plan, threshold)[0]

    def topic_boosts_device(self, question_topics: List[str], chunk_tags_strs: Sequence[str],
                            threshold: float = DEFAULT_THRESHOLD) -> torch.Tensor:
        """fp64 [n] on the matcher's device, enqueued on the current stream; nothing is synchronised"""
        if not self.on_gpu:
            raise RuntimeError("topic_boosts_device needs the matcher on a GPU")
        plan = self._plan(question_topics, chunk_tags_strs)
        if self._fits_kernel(plan, threshold):
            return self._device(plan, threshold)
        return torch.from_numpy(np.asarray(self._host(plan, threshold)[0], dtype=np.float64)).to(self.device)

    def topic_boosts_device_batch(self, question_topics_list: Sequence, chunk_tags_strs_list: Sequence[Sequence],
                                  threshold: float = DEFAULT_THRESHOLD) -> torch.Tensor:
        """topic_boosts_device for several questions at once: fp64 [n_total] on the matcher's device, question q's candidates at
        [sum of the lengths before it, ...), enqueued on the current stream; nothing is synchronised. One plan per question, ONE
        embed call for every string of the batch that has no embedding yet, one upload and one rdx_topic_boost_batch call: per
        question the bits of topic_boosts_device on that question alone. A question beyond the kernel's limits (_fits_kernel) is
        evaluated by the host evaluator, that question only, and its values are copied into place."""
        if not self.on_gpu:
            raise RuntimeError("topic_boosts_device_batch needs the matcher on a GPU")
        topics_list, tags_list = list(question_topics_list), [list(t) for t in chunk_tags_strs_list]
        if len(topics_list) != len(tags_list):
            raise ValueError(f"topic_boosts_device_batch: {len(topics_list)} topic lists for {len(tags_list)} candidate lists")
        plans = [_Plan(t, c) for t, c in zip(topics_list, tags_list)]
        self._ensure([s for plan in plans for s in plan.strings()])
        on_device = [q for q, plan in enumerate(plans) if self._fits_kernel(plan, threshold)]
        dev = self._device_batch([plans[q] for q in on_device], threshold) if on_device else None
        if dev is not None and len(on_device) == sum(1 for plan in plans if len(plan.offsets) > 1):
            return dev                                           # every question that has candidates went to the kernel: its axis is the answer
        pieces, at, where = [], 0, set(on_device)
        for q, plan in enumerate(plans):
            n = len(plan.offsets) - 1
            if q in where:
                pieces.append(dev[at:at + n])
                at += n
            elif n:
                pieces.append(torch.from_numpy(np.asarray(self._host(plan, threshold)[0], dtype=np.float64)).to(self.device))
        return torch.cat(pieces) if pieces else torch.empty((0,), dtype=torch.float64, device=self.device)

    def best_similarities(self, question_topics: List[str], chunk_tags_strs: Sequence[str]) -> List[float]:
        """the best similarity behind each boost (the host evaluator's; the kernel's `best_sim` holds the same bits)"""
        return self._host(self._plan(question_topics, chunk_tags_strs), DEFAULT_THRESHOLD, boosts=False)[1]

    def _plan(self, question_topics, chunk_tags_strs) -> _Plan:
        plan = _Plan(question_topics, chunk_tags_strs)
        self._ensure(plan.strings())
        return plan

    def _fits_kernel(self, plan: _Plan, threshold) -> bool:
        from . import _lib as L
        n = len(plan.offsets) - 1
        return (self.on_gpu and 1 <= n <= L.TOPIC_MAX_N and len(plan.topics) <= L.TOPIC_MAX_TOPICS and plan.max_tags <= L.TOPIC_MAX_TAGS
                and (self._dim is None or self._dim <= L.TOPIC_MAX_DIM) and float(threshold) != 1.0)   # (threshold 1.0: the reference divides by zero, and so does _host)

    def _host(self, plan: _Plan, threshold: float, boosts: bool = True):
        """the kernel's arithmetic on the host -> (boosts, best similarities)"""
        self.stats["host_calls"] += 1
        with self._lock:
            ts = [self._slots.get(t, -1) for t in plan.topics]
            us = [self._slots.get(t, -1) for t in plan.tags]
            a, b = self._rows_host(ts), self._rows_host(us)
        sims = None
        if ts and us:
            sims = dots_kernel_order(a, b)
            sims[np.asarray(ts) < 0, :] = 0.0
            sims[:, np.asarray(us) < 0] = 0.0
        out, bests = [], []
        for c in range(len(plan.offsets) - 1):
            best, prev = 0.0, -1
            for t, u, exact in plan.pairs[plan.offsets[c]:plan.offsets[c + 1]]:
                if t != prev and prev >= 0 and best >= 1.0:
                    break
                prev = t
                if exact:
                    best = 1.0
                    break
                sim = float(sims[t, u])
                if sim > best:
                    best = sim
            bests.append(best)
            if boosts:
                out.append(0.0 if best < threshold else MAX_BOOST * (best - threshold) / (1.0 - threshold))
        return out, bests

    def _upload(self, words: np.ndarray) -> torch.Tensor:
        """int32 host words -> device through the ring of pinned buffers (a pageable copy would park the host behind the stream's work)"""
        buf, slot = self._staging.put(words)
        dev = buf.to(self.device, non_blocking=True)
        slot[1] = self._event()
        return dev

    def _event(self):
        """an event recorded on the current stream of the matcher's device"""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return ev

    def _call_buffers(self, n_sims: int, n: int, want_best: bool):
        """what both device calls are given besides the plan: (table pointer or None, rows, dim, sims, boosts, best or None)"""
        table = self._table.data_ptr() if self._table is not None else None
        sims = torch.empty((max(1, n_sims),), dtype=torch.float64, device=self.device)
        boosts = torch.empty((n,), dtype=torch.float64, device=self.device)
        best = torch.empty((n,), dtype=torch.float64, device=self.device) if want_best else None
        return table, len(self._slots), self._dim or 1, sims, boosts, best

    def _device_batch(self, plans: Sequence[_Plan], threshold: float, want_best: bool = False):
        """rdx_topic_boost_batch on plans that fit the kernel -> fp64 [sum of their candidates] (and the best similarities)"""
        from . import _lib as L
        self.stats["device_calls"] += 1
        nq = len(plans)
        with self._lock, torch.cuda.device(self.device):
            p = pack_plans(plans, lambda t: self._slots.get(t, -1))
            n, T, U, P = int(p["cand_off"][-1]), len(p["topic_slots"]), len(p["tag_slots"]), len(p["pairs"])
            # shape arrays, pinned (the library reads them on the host, the kernels the same words): three int32 arrays, then sim_off (int64, 8-byte aligned)
            pad = (3 * (nq + 1)) % 2
            shape = np.zeros((3 * (nq + 1) + pad + 2 * (nq + 1),), dtype=np.int32)
            shape[:nq + 1], shape[nq + 1:2 * (nq + 1)], shape[2 * (nq + 1):3 * (nq + 1)] = p["topic_off"], p["tag_off"], p["cand_off"]
            shape[3 * (nq + 1) + pad:] = p["sim_off"].view(np.int32)
            pinned, slot = self._shapes.put(shape)
            # everything else in one upload: the slots, then pair_off (int64, 8-byte aligned), then the pair words
            at_off = T + U + (T + U) % 2
            words = np.zeros((at_off + 2 * (n + 1) + P,), dtype=np.int32)
            words[:T], words[T:T + U] = p["topic_slots"], p["tag_slots"]
            words[at_off:at_off + 2 * (n + 1)] = p["pair_off"].view(np.int32)
            words[at_off + 2 * (n + 1):] = p["pairs"]
            d = self._upload(words)
            table, rows, dim, sims, boosts, best = self._call_buffers(int(p["sim_off"][-1]), n, want_best)
            base, sbase = d.data_ptr(), pinned.data_ptr()
            L.check(self._lib.rdx_topic_boost_batch(self.device.index, table, rows, dim, nq,
                                                    sbase, base, sbase + 4 * (nq + 1), base + 4 * T, sbase + 4 * (3 * (nq + 1) + pad),
                                                    sbase + 8 * (nq + 1), base + 4 * at_off, base + 4 * (at_off + 2 * (n + 1)), P,
                                                    float(threshold), MAX_BOOST, sims.data_ptr(), boosts.data_ptr(),
                                                    best.data_ptr() if best is not None else None,
                                                    torch.cuda.current_stream(self.device).cuda_stream))
            slot[1] = self._event()
        return (boosts, best) if want_best else boosts

    def _device(self, plan: _Plan, threshold: float, want_best: bool = False):
        from . import _lib as L
        self.stats["device_calls"] += 1
        n = len(plan.offsets) - 1
        with self._lock, torch.cuda.device(self.device):
            T, U, P = len(plan.topics), len(plan.tags), len(plan.pairs)
            words = np.empty((T + U + n + 1 + P,), dtype=np.int32)
            words[:T] = [self._slots.get(t, -1) for t in plan.topics]
            words[T:T + U] = [self._slots.get(t, -1) for t in plan.tags]
            words[T + U:T + U + n + 1] = plan.offsets
            words[T + U + n + 1:] = [L.topic_pair(t, u, e) for t, u, e in plan.pairs]
            d = self._upload(words)
            table, rows, dim, sims, boosts, best = self._call_buffers(T * U, n, want_best)
            base = d.data_ptr()
            L.check(self._lib.rdx_topic_boost(self.device.index, table, rows, dim,
                                              base, T, base + 4 * T, U, base + 4 * (T + U), base + 4 * (T + U + n + 1), P, n,
                                              float(threshold), MAX_BOOST, sims.data_ptr(), boosts.data_ptr(),
                                              best.data_ptr() if best is not None else None,
                                              torch.cuda.current_stream(self.device).cuda_stream))
        return (boosts, best) if want_best else boosts

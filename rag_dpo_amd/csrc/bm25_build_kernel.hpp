// bm25_build_kernel.hpp — building a BM25 index from text (gfx950): the tokenizer and the term table. Serves BM25Okapi(corpus_tokens)
// in the reference's SummaryBM25Index.build / ChunkBM25Index.build_from_collection (src/rag/bm25_index.py:124, :234) and the
// tokenize_french calls that feed it (:36-52). Included by rdx_bm25_build.hip alone; rag_dpo_amd/bm25_build.py drives it and holds
// the rule's Python model (tokenize_utf8), which the tests compare the kernels against.
//
// Input: the rows' UTF-8 texts concatenated in HBM, one 0x00 byte after each row; row r is text[row_off[r] .. row_off[r + 1] - 1).
// NUL is a separator, so no token runs from one row into the next, and a walk along a token needs no bound but the NUL. The text
// is valid UTF-8 (it comes from str.encode); it is only read.
//
// The rule (bm25_build.py's docstring has the derivation). The word characters W and their normalised bytes:
//   0-9 a-z                                  themselves            A-Z                           byte + 0x20
//   C3 b, bit (b - 0xA0) of BM25_C3_LOWER    themselves            C3 b, bit (b - 0x80) of _UPPER  C3 (b + 0x20)
//   C5 92 / C5 93 (Œ œ)                      C5 93                 C5 B8 (Ÿ)                     C3 BF
//   E2 84 AA (Kelvin sign)                   'k'                   C4 B0 (İ)                     'i', and the token ENDS after it
// Every other character separates. A token is a maximal run of W characters and joining hyphens ('-' between two W characters,
// the break after İ counting as a non-W). It is kept when it has more than one character (characters, not bytes) and its
// normalised bytes are no stop word. One thread looks at one byte: it starts a token when a W character starts there, none ends just
// before it, and no joining hyphen links it to one — one character of look-behind, two across a hyphen. The thread that starts a
// token walks it to its end, which may lie any number of chunks further on.
//
// The term table: open addressing in HBM, BM25 slots a power of two, linear probing, a slot = {rep, first_pos}, both u64.
//   rep        the device address of one occurrence of the term, claimed with ONE 64-bit atomicCAS from 0; the CAS's return value
//              is authoritative. A lane that finds the slot taken compares its token with the occurrence at rep, both normalised
//              on the fly, until both end; equal -> it shares the slot, else it probes on. A term's identity is its bytes, never
//              its hash: the hash (ANDed with hash_mask, all ones in production) only picks the first slot.
//   first_pos  atomicMin of (row << 32) | byte offset of the token in its row: the term's first occurrence. Sorting the occupied
//              slots by it gives rank_bm25's vocabulary order, whichever lane claimed the slot.
// No lane waits for another lane's store: rep points into the TEXT, which was complete before the launch, so a winner has nothing
// left to publish and a loser nothing to wait for. The probe loop is bounded by the table size. A table more than half full raises
// the `full` counter; from then on lanes stop looking terms up and the kernel runs to its end (the host starts over with a larger
// table). Slot reads before the CAS are agent-scope atomic loads (a stale 0 only costs a failed CAS). Every atomic is a vector one.
//
// Limits (checked by rdx_bm25_build_tokenize before anything is enqueued): rows of one build < 2^31, bytes of a row < 2^32,
// slots <= 2^31 (so terms < 2^31).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

constexpr int BM25_TOK_THREADS = 256;
constexpr int BM25_TOK_CHUNK = 256;          // bytes of a row one step of a block covers, one per thread; longer rows loop
constexpr int BM25_TOK_MAX_BLOCKS = 65536;   // rows beyond that share blocks
constexpr int BM25_VOCAB_THREADS = 256;
constexpr int64_t BM25_BUILD_MAX_ROWS = 2147483647;        // rows of one build: a key holds the row in 32 bits, the slot above it
constexpr int64_t BM25_BUILD_MAX_ROW_BYTES = 4294967295;   // first_pos holds the byte offset in 32 bits
constexpr int64_t BM25_BUILD_MAX_SLOTS = 2147483648;
constexpr uint32_t BM25_C3_LOWER = 0x9A10CFD5u;            // à â ä æ ç è é ê ë î ï ô ù û ü ÿ as bits of (second byte - 0xA0)
constexpr uint32_t BM25_C3_UPPER = 0x1A10CFD5u;            // their capitals as bits of (second byte - 0x80); bit 31 would be ß
enum { BM25_CNT_TERMS = 0, BM25_CNT_TOKENS = 1, BM25_CNT_FULL = 2, BM25_CNT_OVERFLOW = 3, BM25_N_COUNTERS = 4 };

typedef unsigned long long bm25_u64;

struct Bm25Slot {
    bm25_u64 rep;         // 0 = free
    bm25_u64 first_pos;   // ~0 until a token arrives
};

// the stop words of more than one character (rag_dpo_amd/bm25.py STOPWORDS; one-character tokens are dropped anyway): normalised
// bytes packed little-endian into 64 bits, ascending = bm25_build.stopword_keys(), pinned by tests/test_bm25_build_model.py
constexpr int BM25_N_STOPWORDS = 102;
static __device__ const bm25_u64 BM25_STOPWORDS[BM25_N_STOPWORDS] = {
    0x616cull, 0x616dull, 0x6173ull, 0x6174ull, 0x6563ull, 0x6564ull,
    0x656aull, 0x656cull, 0x656eull, 0x6573ull, 0x696eull, 0x6973ull,
    0x6c69ull, 0x6e65ull, 0x6e6full, 0x6e75ull, 0x7465ull, 0x7561ull,
    0x7564ull, 0x756full, 0x7574ull, 0x656e75ull, 0x657571ull, 0x697571ull,
    0x6e6f6dull, 0x6e6f73ull, 0x6e6f74ull, 0x726163ull, 0x726170ull, 0x727573ull,
    0x736170ull, 0x736563ull, 0x736564ull, 0x73656cull, 0x73656dull, 0x736573ull,
    0x736574ull, 0x736c69ull, 0x746563ull, 0x747365ull, 0x756570ull, 0x787561ull,
    0xb9c36full, 0x63657661ull, 0x636e6f64ull, 0x656c6c65ull, 0x696f7571ull, 0x6c657571ull,
    0x6e656962ull, 0x6e656972ull, 0x706f7274ull, 0x7275656cull, 0x72756f70ull, 0x7369616dull,
    0x736e6164ull, 0x736e6173ull, 0x73726576ull, 0x73726f6cull, 0x73756c70ull, 0x73756f6eull,
    0x73756f73ull, 0x73756f74ull, 0x73756f76ull, 0x74696166ull, 0x746e6f64ull, 0x746e6f73ull,
    0x74756570ull, 0x74756f74ull, 0x7a656863ull, 0x656d6d6f63ull, 0x656daac36dull, 0x6572696166ull,
    0x6572746e65ull, 0x6572746f6eull, 0x6572746f76ull, 0x6572747561ull, 0x657274aac3ull, 0x6574746563ull,
    0x6574756f74ull, 0x69736e6961ull, 0x6973737561ull, 0x72696f7661ull, 0x73656c6c65ull, 0x736c657571ull,
    0x73726f6c61ull, 0x737275656cull, 0x73a8c37274ull, 0x746e617661ull, 0x746e617961ull, 0x7a65737361ull,
    0xa9c374a9c3ull, 0x656c6c657571ull, 0x65726f636e65ull, 0x657571616863ull, 0x736572747561ull, 0x736574756f74ull,
    0x7369616d616aull, 0x736975706564ull, 0x73a8c3727061ull, 0xa0c36aa9c364ull, 0x73656c6c657571ull, 0x746e61646e6570ull,
};

struct Bm25Char {
    uint32_t norm;   // the normalised bytes, first byte lowest
    int take;        // bytes of text
    int nb;          // normalised bytes (1 or 2)
    bool brk;        // the token ends after this character (İ)
};

__device__ __forceinline__ bool bm25_alnum(uint32_t b) { return b - '0' <= 9u || b - 'a' < 26u || b - 'A' < 26u; }

// the word character that starts at p, if one does. Reads p[1] only behind a lead byte and p[2] only behind E2 84, so never past
// the NUL that ends the row. A continuation byte starts none, so any byte position may be asked.
__device__ __forceinline__ bool bm25_word_char(const uint8_t* p, Bm25Char& c) {
    const uint32_t b0 = p[0];
    c.brk = false;
    c.take = 1;
    c.nb = 1;
    if (b0 < 0x80) {
        c.norm = b0 - 'A' < 26u ? b0 + 0x20 : b0;
        return bm25_alnum(b0);
    }
    if (b0 != 0xC3 && b0 != 0xC4 && b0 != 0xC5 && b0 != 0xE2) return false;
    const uint32_t b1 = p[1];
    c.take = 2;
    if (b0 == 0xC3) {
        c.nb = 2;
        if (b1 >= 0xA0 && b1 <= 0xBF) {
            c.norm = 0xC3u | b1 << 8;
            return BM25_C3_LOWER >> (b1 - 0xA0) & 1u;
        }
        if (b1 >= 0x80 && b1 <= 0x9F) {
            c.norm = 0xC3u | (b1 + 0x20) << 8;
            return BM25_C3_UPPER >> (b1 - 0x80) & 1u;
        }
        return false;
    }
    if (b0 == 0xC5) {
        c.nb = 2;
        c.norm = b1 == 0xB8 ? 0xBFC3u : 0x93C5u;
        return b1 == 0x92 || b1 == 0x93 || b1 == 0xB8;
    }
    if (b0 == 0xC4) {
        c.norm = 'i';
        c.brk = true;
        return b1 == 0xB0;
    }
    c.norm = 'k';
    c.take = 3;
    return b1 == 0x84 && p[2] == 0xAA;
}

// does a word character without a forced break end just before row[q]? Never reads before row[0].
__device__ __forceinline__ bool bm25_word_ends_at(const uint8_t* row, int64_t q) {
    if (q < 1) return false;
    const uint32_t b = row[q - 1];
    if (b < 0x80) return bm25_alnum(b);
    Bm25Char c;
    if (q >= 2) {
        const uint32_t lead = row[q - 2];
        if (lead == 0xC3 || lead == 0xC5) return bm25_word_char(row + q - 2, c);
    }
    if (q >= 3 && row[q - 3] == 0xE2) return bm25_word_char(row + q - 3, c);
    return false;
}

__device__ __forceinline__ bool bm25_starts_token(const uint8_t* row, int64_t i) {
    Bm25Char c;
    if (!bm25_word_char(row + i, c) || bm25_word_ends_at(row, i)) return false;
    return !(i >= 1 && row[i - 1] == '-' && bm25_word_ends_at(row, i - 1));
}

// the next character of the token p stands in (first call: p = the token's start): a word character, or a hyphen with a word
// character behind it. false = the token has ended. brk carries İ's forced break from one call to the next.
__device__ __forceinline__ bool bm25_tok_next(const uint8_t*& p, bool& brk, Bm25Char& c) {
    if (brk) return false;
    if (bm25_word_char(p, c)) {
        p += c.take;
        brk = c.brk;
        return true;
    }
    if (p[0] != '-') return false;
    Bm25Char after;
    if (!bm25_word_char(p + 1, after)) return false;
    c.norm = '-';
    c.take = c.nb = 1;
    p += 1;
    return true;
}

// are the tokens that start at a and at b the same normalised bytes? (a normalised character is 1 byte < 0x80 or 2 bytes with a
// lead byte first, so equal characters <=> equal bytes)
__device__ __forceinline__ bool bm25_same_token(const uint8_t* a, const uint8_t* b) {
    bool brk_a = false, brk_b = false;
    for (;;) {
        Bm25Char ca, cb;
        const bool more_a = bm25_tok_next(a, brk_a, ca), more_b = bm25_tok_next(b, brk_b, cb);
        if (more_a != more_b) return false;
        if (!more_a) return true;
        if (ca.norm != cb.norm) return false;
    }
}

__device__ __forceinline__ bool bm25_is_stopword(bm25_u64 packed) {
    int lo = 0, hi = BM25_N_STOPWORDS;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (BM25_STOPWORDS[mid] < packed) lo = mid + 1;
        else hi = mid;
    }
    return lo < BM25_N_STOPWORDS && BM25_STOPWORDS[lo] == packed;
}

__device__ __forceinline__ bm25_u64 bm25_load(const bm25_u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot of the term whose occurrence starts at tok (hash h, already masked), or -1 when the table cannot take it
__device__ __forceinline__ int64_t bm25_find_slot(Bm25Slot* table, bm25_u64 slot_mask, bm25_u64 h, const uint8_t* tok, bm25_u64 pos,
                                                  bm25_u64* counters) {
    if (bm25_load(&counters[BM25_CNT_FULL])) return -1;   // the build is lost: do not crawl through a crowded table
    bm25_u64 s = h & slot_mask;
    for (bm25_u64 probe = 0; probe <= slot_mask; ++probe, s = (s + 1) & slot_mask) {
        bm25_u64 rep = bm25_load(&table[s].rep);
        if (rep == 0) {
            rep = atomicCAS(&table[s].rep, 0ull, (bm25_u64)tok);
            if (rep == 0) {   // claimed: this occurrence represents the term
                rep = (bm25_u64)tok;
                if (2 * (atomicAdd(&counters[BM25_CNT_TERMS], 1ull) + 1) > slot_mask + 1) atomicMax(&counters[BM25_CNT_FULL], 1ull);
            }
        }
        if (rep == (bm25_u64)tok || bm25_same_token((const uint8_t*)rep, tok)) {
            if (bm25_load(&table[s].first_pos) > pos) atomicMin(&table[s].first_pos, pos);   // common terms are hot: read first
            return (int64_t)s;
        }
    }
    atomicMax(&counters[BM25_CNT_FULL], 1ull);
    return -1;
}

__global__ __launch_bounds__(256) void k_bm25_table_init(Bm25Slot* table, int64_t slots) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (int64_t)gridDim.x * blockDim.x) {
        table[s].rep = 0;
        table[s].first_pos = ~0ull;
    }
}

// One block per row (rows beyond the grid share blocks), one thread per byte of a chunk. For every kept token: its term's slot, and
// one key (slot << 32) | (row_base + row) into the row's own stretch keys[key_off[r] .. key_off[r + 1]), which holds (len + 1) / 3
// keys — a kept token has >= 2 bytes and a separator before the next, or ends in İ and has >= 3 — in any order (the host sorts);
// the rest of the stretch is filled with -1. doc_len[r] = kept tokens of the row.
__global__ __launch_bounds__(BM25_TOK_THREADS) void k_bm25_tok(const uint8_t* __restrict__ text, const int64_t* __restrict__ row_off,
                                                               const int64_t* __restrict__ key_off, int64_t n_rows, int64_t row_base,
                                                               Bm25Slot* table, bm25_u64 slot_mask, bm25_u64 hash_mask,
                                                               int64_t* __restrict__ keys, int32_t* __restrict__ doc_len,
                                                               bm25_u64* counters) {
    __shared__ int s_kept;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const uint8_t* row = text + row_off[r];
        const int64_t len = row_off[r + 1] - row_off[r] - 1;
        const int64_t kbase = key_off[r], kcap = key_off[r + 1] - kbase;
        if (threadIdx.x == 0) s_kept = 0;
        __syncthreads();
        for (int64_t c0 = 0; c0 < len; c0 += BM25_TOK_CHUNK) {
            const int64_t i = c0 + threadIdx.x;
            if (i >= len || !bm25_starts_token(row, i)) continue;
            // walk the token: characters, FNV-1a of the normalised bytes, and the bytes themselves while they fit 64 bits
            const uint8_t* p = row + i;
            bool brk = false;
            Bm25Char c;
            int64_t chars = 0, nbytes = 0;
            bm25_u64 h = 0xcbf29ce484222325ull, packed = 0;
            while (bm25_tok_next(p, brk, c)) {
                for (int b = 0; b < c.nb; ++b) {
                    const bm25_u64 byte = (c.norm >> (8 * b)) & 0xFFu;
                    h = (h ^ byte) * 0x100000001b3ull;
                    if (nbytes < 8) packed |= byte << (8 * nbytes);
                    ++nbytes;
                }
                ++chars;
            }
            if (chars < 2 || (nbytes <= 8 && bm25_is_stopword(packed))) continue;
            h ^= h >> 33;   // FNV's low bits are weak: fold the high ones in before the mask takes the low ones
            h *= 0xff51afd7ed558ccdull;
            h ^= h >> 33;
            const int64_t slot = bm25_find_slot(table, slot_mask, h & hash_mask, row + i, (bm25_u64)(row_base + r) << 32 | (bm25_u64)i,
                                                counters);
            if (slot < 0) continue;
            const int at = atomicAdd(&s_kept, 1);
            if (at < kcap) keys[kbase + at] = slot << 32 | (row_base + r);
            else atomicMax(&counters[BM25_CNT_OVERFLOW], 1ull);   // cannot happen (the bound above); never write past the stretch
        }
        __syncthreads();
        const int kept = s_kept;
        for (int64_t j = (int64_t)kept + threadIdx.x; j < kcap; j += BM25_TOK_THREADS) keys[kbase + j] = -1;
        if (threadIdx.x == 0) {
            doc_len[r] = kept;
            if (kept) atomicAdd(&counters[BM25_CNT_TOKENS], (bm25_u64)kept);
        }
        __syncthreads();   // s_kept is reset for the next row
    }
}

// One thread per term t, slot slots[t]: the normalised bytes of the term's representative occurrence (every occurrence of a term
// normalises to the same bytes). arena == nullptr: term_off[t] = the term's length in bytes. Otherwise the bytes go to
// arena[term_off[t] .. term_off[t + 1]), cut at that stretch and at arena_bytes.
__global__ __launch_bounds__(BM25_VOCAB_THREADS) void k_bm25_vocab(const Bm25Slot* __restrict__ table, bm25_u64 slot_mask,
                                                                   const int32_t* __restrict__ slots, int64_t n_terms, int64_t* term_off,
                                                                   uint8_t* __restrict__ arena, int64_t arena_bytes) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_terms) return;
    const bm25_u64 s = (bm25_u64)(uint32_t)slots[t];
    const uint8_t* p = s <= slot_mask ? (const uint8_t*)table[s].rep : nullptr;
    int64_t at = 0, end = 0;
    if (arena) {
        at = term_off[t];
        end = term_off[t + 1] < arena_bytes ? term_off[t + 1] : arena_bytes;
        if (at < 0) at = end;
    }
    int64_t nbytes = 0;
    bool brk = false;
    Bm25Char c;
    while (p && bm25_tok_next(p, brk, c)) {
        for (int b = 0; b < c.nb; ++b, ++nbytes)
            if (arena && at + nbytes < end) arena[at + nbytes] = (uint8_t)(c.norm >> (8 * b));
    }
    if (!arena) term_off[t] = nbytes;
}

}  // namespace rdx

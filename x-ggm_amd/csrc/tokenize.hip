// WordPiece tokenisation of a whole corpus in ONE launch (contract: xggm_tokenize_wordpiece in xggm.h): what
// BertTokenizer.tokenize(sent.strip()) + convert_sents_to_features do per sentence on the host (src/lxrt/tokenization.py:72-348,
// src/lxrt/entry.py:37-72), from packed UTF-8 bytes and host-built tables.  Integer work only: every output is exact.
//
// Mapping: one THREAD per sentence, workgroups of one wave.  A sentence is a serial automaton over its bytes (decode, clean,
// fold, split, greedy longest match); its data-dependent chains are table lookups, so throughput comes from many sentences
// in flight, not from lanes co-operating on one 50-byte string ("Tokenise on the device").  The only
// runtime-indexed per-sentence scratch -- the folded code points of the word being matched, at most 100 -- lives in LDS,
// one column per lane (s_word[i][lane]: lanes of a wave at the same i hit 64 different banks).  Substring hashes need no
// prefix array: the hash of [s, e - 1) follows from that of [s, e) by one subtraction and one multiplication with the
// multiplier's inverse modulo 2^64.
#include "common.h"
#include "xggm.h"

namespace {
constexpr int NT = 64;                         // threads (= sentences) per workgroup
constexpr int MAXW = XGGM_TOKENIZE_MAX_WORD;   // max_input_chars_per_word (src/lxrt/tokenization.py:294)
constexpr uint64_t HP = XGGM_TOKENIZE_HASH_MUL, HPINV = XGGM_TOKENIZE_HASH_MUL_INV;
static_assert(HP * HPINV == 1ull, "HASH_MUL_INV is the inverse of HASH_MUL modulo 2^64");
enum { ACT_KEEP = 0, ACT_DROP = 1, ACT_SPACE = 2, ACT_CJK = 3, ACT_HOST = 4 };

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// the folded code points of the word in flight, one LDS column per sentence
struct Word {
    uint32_t* col;  // &s_word[0][lane]
    int n;          // code points so far (only the first MAXW are stored: a longer word is [UNK] whatever it holds)
    __device__ __forceinline__ uint32_t get(int i) const { return col[i * NT]; }
    __device__ __forceinline__ void push(uint32_t c) {
        if (n < MAXW) col[n * NT] = c;
        ++n;
    }
};

// strict UTF-8 (RFC 3629: no overlong forms, no surrogates, nothing past U+10FFFF); reads bytes of [p, end) only.
// -> bytes consumed; 0: malformed or cut off by the sentence's end
__device__ __forceinline__ int decode_utf8(const uint8_t* b, int64_t p, int64_t end, uint32_t& cp) {
    const uint32_t b0 = b[p];
    if (b0 < 0x80u) {
        cp = b0;
        return 1;
    }
    int need;
    uint32_t lo = 0x80u, hi = 0xBFu;
    if (b0 >= 0xC2u && b0 <= 0xDFu) {
        need = 1;
        cp = b0 & 0x1Fu;
    } else if (b0 >= 0xE0u && b0 <= 0xEFu) {
        need = 2;
        cp = b0 & 0x0Fu;
        if (b0 == 0xE0u) lo = 0xA0u;
        if (b0 == 0xEDu) hi = 0x9Fu;
    } else if (b0 >= 0xF0u && b0 <= 0xF4u) {
        need = 3;
        cp = b0 & 0x07u;
        if (b0 == 0xF0u) lo = 0x90u;
        if (b0 == 0xF4u) hi = 0x8Fu;
    } else {
        return 0;
    }
    if (p + need >= end) return 0;
    for (int i = 1; i <= need; ++i) {
        const uint32_t c = b[p + i];
        if (c < lo || c > hi) return 0;
        lo = 0x80u;
        hi = 0xBFu;
        cp = (cp << 6) | (c & 0x3Fu);
    }
    return need + 1;
}

struct Tok {
    const xggm_tokenize_args& a;
    int32_t* row32;  // ids row or NULL
    int64_t* row64;  // ids row of the int64 block or NULL
    int L;           // T - 2
    int cnt;         // tokens of the sentence so far, <= L

    __device__ __forceinline__ void put(int k, int32_t id) const {  // token k of the sentence sits behind [CLS]
        if (row32) row32[1 + k] = id;
        if (row64) row64[1 + k] = id;
    }

    // id of the piece w[s, e) with hash h in `slots`, -1: absent.  A slot is {hash >> 32, id, blob offset, length}; a hit
    // counts only after the code points compare equal, an id of -1 ends the probe sequence (open addressing, linear).
    __device__ int lookup(const uint32_t* slots, int64_t cap, uint64_t h, const Word& w, int s, int e) const {
        const uint32_t tag = (uint32_t)(h >> 32), len = (uint32_t)(e - s);
        uint64_t i = (h ^ (h >> 32)) & (uint64_t)(cap - 1);
        for (int64_t probes = 0; probes < cap; ++probes) {
            const u4 sl = *reinterpret_cast<const u4*>(slots + 4 * i);
            if ((int32_t)sl[1] < 0) return -1;
            if (sl[0] == tag && sl[3] == len && (int64_t)sl[2] + len <= a.n_blob) {
                uint32_t j = 0;
                while (j < len && a.blob[sl[2] + j] == w.get(s + (int)j)) ++j;
                if (j == len) return (int32_t)sl[1];
            }
            i = (i + 1) & (uint64_t)(cap - 1);
        }
        return -1;
    }

    // WordpieceTokenizer.tokenize of one word (:299-348).  Pieces are written where they would go and count only once the
    // whole word has matched: a word with an unmatched remainder is ONE [UNK], also when its first pieces filled the row.
    __device__ void wordpiece(Word& w) {
        const int len = w.n;
        w.n = 0;
        if (len == 0 || cnt >= L) return;
        if (len > MAXW) {
            put(cnt++, a.unk_id);
            return;
        }
        int s = 0, pieces = 0;
        while (s < len) {
            uint64_t h = 0;
            for (int i = s; i < len; ++i) h = h * HP + (w.get(i) + 1u);
            int e = len, id = -1;
            while (e > s) {
                id = s ? lookup(a.cont_slots, a.cont_cap, h, w, s, e) : lookup(a.init_slots, a.init_cap, h, w, s, e);
                if (id >= 0) break;
                h = (h - (w.get(e - 1) + 1u)) * HPINV;
                --e;
            }
            if (id < 0) {
                put(cnt++, a.unk_id);
                return;
            }
            if (cnt + pieces < L) put(cnt + pieces, id);
            ++pieces;
            s = e;
        }
        cnt = min(cnt + pieces, L);
    }
};

// sentence `row` with its word column `col` (stride NT) -> everything but the count of flagged rows; returns the row's flag
__device__ uint32_t tokenize_row(const xggm_tokenize_args& a, int64_t row, uint32_t* col) {
    const int T = a.T;
    // the sentence's bytes, held inside the buffer whatever the device copy of the offsets says
    int64_t p = a.offsets[row], end = a.offsets[row + 1];
    p = p < 0 ? 0 : (p > a.n_bytes ? a.n_bytes : p);
    end = end < p ? p : (end > a.n_bytes ? a.n_bytes : end);

    Tok t = {a, a.ids ? a.ids + row * T : nullptr, a.block ? a.block + row * T : nullptr, T - 2, 0};
    Word w = {col, 0};
    uint32_t host = 0;
    bool fresh = true;  // the next kept character opens a whitespace token
    while (p < end && t.cnt < t.L) {
        uint32_t cp;
        const int nb = decode_utf8(a.bytes, p, end, cp);
        if (nb == 0) {  // malformed: the row goes to the host; here the byte is dropped like U+FFFD
            host = 1;
            ++p;
            continue;
        }
        const uint32_t ent = a.cp_table[cp];
        uint32_t act = ent & 7u;
        if (act == ACT_HOST) {
            host = 1;
            act = ACT_KEEP;
        }
        if (act == ACT_DROP) {
            p += nb;
            continue;
        }
        if (act == ACT_SPACE) {
            t.wordpiece(w);
            fresh = true;
            p += nb;
            continue;
        }
        if (act == ACT_KEEP && fresh && a.n_never > 0) {
            // a whitespace token that IS a never_split token passes through unfolded and unsplit (:200-204, :222-223): follow the
            // candidates that still match, character by character, to the token's end
            uint32_t alive = 0;
            for (int k = 0; k < a.n_never; ++k)
                if (a.never_off[k + 1] > a.never_off[k] && a.never_cps[a.never_off[k]] == cp) alive |= 1u << k;
            if (alive) {
                int64_t q = p + nb;
                int j = 1;
                while (alive && q < end) {
                    uint32_t c2;
                    const int nb2 = decode_utf8(a.bytes, q, end, c2);
                    if (nb2 == 0) {  // a malformed byte inside the token: dropped and flagged, as in the main loop
                        host = 1;
                        ++q;
                        continue;
                    }
                    const uint32_t act2 = a.cp_table[c2] & 7u;
                    if (act2 == ACT_DROP) {
                        q += nb2;
                        continue;
                    }
                    if (act2 == ACT_SPACE || act2 == ACT_CJK) break;
                    uint32_t still = 0;
                    for (int k = 0; k < a.n_never; ++k)
                        if ((alive >> k & 1u) && a.never_off[k] + j < a.never_off[k + 1] && a.never_cps[a.never_off[k] + j] == c2)
                            still |= 1u << k;
                    alive = still;
                    ++j;
                    q += nb2;
                }
                int hit = -1;
                for (int k = 0; k < a.n_never; ++k)
                    if ((alive >> k & 1u) && a.never_off[k + 1] - a.never_off[k] == j) hit = k;
                if (hit >= 0) {  // the bytes behind p up to q hold nothing but this token and dropped characters
                    for (int i = 0; i < j; ++i) w.push(a.never_cps[a.never_off[hit] + i]);
                    t.wordpiece(w);
                    p = q;
                    continue;  // fresh stays true: q is the sentence's end, a space or a CJK character
                }
            }
        }
        if (act == ACT_CJK) t.wordpiece(w);  // a CJK character is a whitespace token of its own (:242-253)
        // lower-case, NFD, drop Mn: the table's folded sequence; then _run_split_on_punc (:209-240)
        const uint32_t nf = (ent >> 3) & 3u, payload = ent >> 8;
        for (uint32_t f = 0; f < nf; ++f) {
            uint32_t c = payload;
            if (nf > 1) c = (int64_t)payload + f < a.n_ext ? a.cp_ext[payload + f] : 0xFFFDu;
            if (ent >> (5 + f) & 1u) {
                t.wordpiece(w);
                w.push(c);
                t.wordpiece(w);
            } else {
                w.push(c);
            }
        }
        fresh = act == ACT_CJK;
        if (act == ACT_CJK) t.wordpiece(w);
        p += nb;
    }
    t.wordpiece(w);

    // [CLS] tokens [SEP], zero padded; mask and segment ids of convert_sents_to_features (src/lxrt/entry.py:57-70)
    const int n_tok = t.cnt + 2;
    if (t.row32) {
        t.row32[0] = a.cls_id;
        t.row32[n_tok - 1] = a.sep_id;
        for (int i = n_tok; i < T; ++i) t.row32[i] = 0;
    }
    if (t.row64) {
        int64_t* mask = t.row64 + a.n * T;
        int64_t* seg = mask + a.n * T;
        t.row64[0] = a.cls_id;
        t.row64[n_tok - 1] = a.sep_id;
        for (int i = n_tok; i < T; ++i) t.row64[i] = 0;
        for (int i = 0; i < T; ++i) {
            mask[i] = i < n_tok;
            seg[i] = 0;
        }
    }
    if (a.len) a.len[row] = n_tok;
    if (a.flags) a.flags[row] = (uint8_t)host;
    return host;
}

__global__ __launch_bounds__(NT) void tokenize_kernel(const xggm_tokenize_args a) {
    __shared__ uint32_t s_word[MAXW][NT];
    const int64_t row = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (row >= a.n) return;  // no barrier anywhere: a thread is on its own
    if (tokenize_row(a, row, &s_word[0][threadIdx.x]) && a.flagged) atomicAdd(a.flagged, 1);
}

bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
bool aligned(const void* p, uintptr_t n) { return (uintptr_t)p % n == 0; }
}  // namespace

extern "C" size_t xggm_tokenize_workspace_bytes(int64_t n, int T) {
    (void)n;
    (void)T;
    return 0;  // the word in flight lives in LDS (MAXW x 64 dwords per workgroup): nothing for the caller to provide
}

extern "C" int xggm_tokenize_wordpiece(const xggm_tokenize_args* args, hipStream_t st) {
    const char* who = "xggm_tokenize_wordpiece";
    XGGM_REQUIRE(args, "%s: null argument struct", who);
    const xggm_tokenize_args& a = *args;
    XGGM_REQUIRE(a.n >= 1, "%s: n=%lld sentences, at least 1 expected", who, (long long)a.n);
    XGGM_REQUIRE(a.T >= 2, "%s: T=%d leaves no room for [CLS] and [SEP] (T >= 2)", who, a.T);
    XGGM_REQUIRE(a.n * (int64_t)a.T < (1ll << 40), "%s: n T must stay below 2^40", who);
    XGGM_REQUIRE(a.n_bytes >= 0 && (a.bytes || a.n_bytes == 0), "%s: null bytes with n_bytes=%lld", who, (long long)a.n_bytes);
    XGGM_REQUIRE(a.offsets && a.host_offsets, "%s: null offsets (device) or host_offsets (their host copy)", who);
    XGGM_REQUIRE(a.cp_table && a.blob && a.init_slots && a.cont_slots, "%s: null table (cp_table, blob, init_slots, cont_slots)", who);
    XGGM_REQUIRE(a.n_ext >= 0 && (a.cp_ext || a.n_ext == 0) && a.n_blob >= 0 && a.n_blob < (1ll << 32),
                 "%s: null cp_ext with n_ext=%lld, or n_blob=%lld outside [0, 2^32)", who, (long long)a.n_ext, (long long)a.n_blob);
    XGGM_REQUIRE(pow2(a.init_cap) && pow2(a.cont_cap), "%s: table capacity %lld / %lld is not a power of two", who,
                 (long long)a.init_cap, (long long)a.cont_cap);
    XGGM_REQUIRE(a.n_never >= 0 && a.n_never <= XGGM_TOKENIZE_MAX_NEVER && (a.n_never == 0 || (a.never_cps && a.never_off)),
                 "%s: n_never=%d outside [0, %d], or null never_cps / never_off", who, a.n_never, XGGM_TOKENIZE_MAX_NEVER);
    XGGM_REQUIRE(a.ids || a.block || a.len || a.flags || a.flagged, "%s: every output pointer is null", who);
    XGGM_REQUIRE(aligned(a.offsets, 8) && aligned(a.block, 8) && aligned(a.ids, 4) && aligned(a.len, 4) && aligned(a.flagged, 4),
                 "%s: misaligned pointer (offsets, block: 8 bytes; ids, len, flagged: 4 bytes)", who);
    XGGM_REQUIRE(aligned(a.init_slots, 16) && aligned(a.cont_slots, 16) && aligned(a.cp_table, 4) && aligned(a.cp_ext, 4) &&
                     aligned(a.blob, 4) && aligned(a.never_cps, 4) && aligned(a.never_off, 4),
                 "%s: misaligned table (slots: 16 bytes; cp_table, cp_ext, blob, never_cps, never_off: 4 bytes)", who);
    for (int64_t i = 0; i <= a.n; ++i) {
        const int64_t o = a.host_offsets[i];
        XGGM_REQUIRE(o >= (i ? a.host_offsets[i - 1] : 0), "%s: offsets[%lld]=%lld is not monotonic (they start at >= 0 and never fall)",
                     who, (long long)i, (long long)o);
        XGGM_REQUIRE(o <= a.n_bytes, "%s: offsets[%lld]=%lld lies past n_bytes=%lld", who, (long long)i, (long long)o, (long long)a.n_bytes);
    }
    XGGM_REQUIRE(ceil_div64(a.n, NT) < (1ll << 31), "%s: n=%lld needs too many workgroups", who, (long long)a.n);
    hipLaunchKernelGGL(tokenize_kernel, dim3((unsigned)ceil_div64(a.n, NT)), dim3(NT), 0, st, a);
    return xggm_check_launch(who);
}

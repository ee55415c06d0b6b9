// Bottom-up feature TSVs decoded on the device (contract: xggm_tsv_decode in xggm.h): the six base64 fields of n lines of
// `train2014_obj36.tsv`-style text, which the host reads with base64.b64decode + np.frombuffer (src/utils.py:41-52) and
// normalises per item (src/pretrain/lxmert_data.py:165-171, src/vqa/vqacpv2_data.py:108-117), become rows of the stores'
// image tables in ONE launch.  Integer and bit work only (the one division is correctly rounded): every output is exact.
//
// Mapping: one WORKGROUP of 256 threads per line, so that a line's flag word has one owner and nothing but the two counters
// is ever an atomic.  The features field (99.5 % of a 36 x 2048 line) goes through in slabs of 256 units; a unit is 128
// characters = 96 bytes = 24 fp32, one thread's work, stored as six (fp32) or three (bf16) 16-byte stores.
//   stage   every thread fetches eight aligned 16-byte words of the slab (coalesced; thread 0 a ninth, the word behind it) and
//           writes them to LDS as they are.  The words of slab s + 1 are in flight while slab s is decoded (36 VGPRs).
//   LDS     unit u owns the nine words at byte 144 u: its eight, and a copy of the next unit's first, which holds the tail of
//           its characters when the field does not start on a word.  With a stride of 36 dwords the nine ds_read_b128 of a
//           thread are 16-byte aligned and the 16 lanes of a ds_read_b128 group fall on 16 different bank quads (9 u mod 16 is
//           a permutation): no conflicts.  The field's start modulo 16 is uniform per line, so the byte-align step is four
//           selects on a uniform condition and one v_alignbyte per dword.  Characters map to sextets through a 256-byte LDS
//           table: 64 dwords, one per bank, so two lanes either share a dword (broadcast) or hit different banks.
//   decode  four characters -> 24 bits -> three bytes; four quads -> three little-endian dwords, all register-indexed.
// The five small fields (at most 2 KB each for O = 128) are decoded afterwards by the same workgroup: one thread per quad
// into LDS bytes, one thread per element out of them.  Stores of a thread's 96 output bytes are 16 bytes wide at a lane
// stride of 96 (fp32) or 48 (bf16) bytes; the L2 merges them.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), the same for tsv_decode_kernel<true> and <false>:
//   VGPRs 231, AGPRs 0, SGPRs 106, LDS 37136 bytes per workgroup, scratch 0, occupancy 2 waves per SIMD (two workgroups per
//   CU).  The compiler spends the registers on hoisting a unit's 128 table reads; capped at 128 VGPRs it spills (420 bytes
//   of scratch per lane), so the cap is not set.
#include "common.h"
#include "xggm.h"

namespace {
constexpr int NT = 256;             // threads per workgroup = units per slab
constexpr int UNIT_BYTES = 96;      // bytes they decode to
constexpr int UNIT_STRIDE = 144;    // LDS bytes between two units' characters (36 dwords: see above)
constexpr int NF = XGGM_TSV_FIELDS, ND = XGGM_TSV_DESC;
constexpr int F_OBJ_ID = 0, F_OBJ_CONF = 1, F_ATTR_ID = 2, F_ATTR_CONF = 3, F_BOXES = 4, F_FEATS = 5;
constexpr uint32_t BAD_CHAR = 1u, BAD_LEN = 2u, BAD_ID = 4u, BAD_BOX = 8u, NONFINITE = 16u;
constexpr uint32_t T_PAD = 0x40u, T_BAD = 0x80u;  // table entries of '=' and of everything outside the alphabet

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct Field {
    int64_t off;   // first character, held inside the text whatever the device copy of the descriptor says
    int bytes;     // bytes the field decodes to for this O, F
    int quads;     // ceil(bytes / 3): the field is 4 * quads characters
    int pad;       // '=' at the end of the last quad
    bool dead;     // wrong length: nothing is decoded, the outputs are zeros
};

__device__ __forceinline__ Field field_of(const xggm_tsv_decode_args& a, const int64_t* d, int f, int bytes) {
    int64_t off = d[2 * f], len = d[2 * f + 1];
    off = off < 0 ? 0 : (off > a.n_bytes ? a.n_bytes : off);
    len = len < 0 ? 0 : (len > a.n_bytes - off ? a.n_bytes - off : len);
    Field r;
    r.off = off;
    r.bytes = bytes;
    r.quads = (bytes + 2) / 3;
    r.pad = r.quads * 3 - bytes;
    r.dead = len != 4 * (int64_t)r.quads;
    return r;
}

// four table entries -> the quad's 24 bits as bytes b0 | b1 << 8 | b2 << 16; `bad` when an entry does not belong where it
// stands: '=' only in the last `pad` places of the field's last quad, and nothing else there
__device__ __forceinline__ uint32_t quad_bytes(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, int pad, bool& bad) {
    const uint32_t w2 = pad >= 2 ? T_PAD : 0u, w3 = pad >= 1 ? T_PAD : 0u;
    bad = ((t0 | t1) & 0xC0u) != 0u || (t2 & 0xC0u) != w2 || (t3 & 0xC0u) != w3;
    const uint32_t v = (t0 & 63u) << 18 | (t1 & 63u) << 12 | (t2 & 63u) << 6 | (t3 & 63u);
    return __builtin_bswap32(v << 8);
}

__device__ __forceinline__ uint16_t bf16_rne(uint32_t x) {  // torch.Tensor.to(torch.bfloat16)
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}

// the aligned 16-byte word `w` of the text, zeros where it would leave the allocation
__device__ __forceinline__ u4 load_word(const xggm_tsv_decode_args& a, int64_t w) {
    if (w < 0 || 16 * w + 16 > a.alloc_bytes) return (u4){0u, 0u, 0u, 0u};
    return reinterpret_cast<const u4*>(a.text)[w];
}

template <bool BF16>
__global__ __launch_bounds__(NT) void tsv_decode_kernel(const xggm_tsv_decode_args a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[NT * UNIT_STRIDE];
    __shared__ __attribute__((aligned(16))) uint8_t s_tab[256];
    const int tid = threadIdx.x;
    const int64_t line = blockIdx.x, row = a.row0 + line;
    const int64_t* d = a.desc + line * ND;
    const int O = a.O, F = a.F;
    uint32_t flag = 0;

    {  // the alphabet of RFC 4648 section 4
        const int c = tid;
        uint32_t t = T_BAD;
        if (c >= 'A' && c <= 'Z') t = c - 'A';
        if (c >= 'a' && c <= 'z') t = c - 'a' + 26;
        if (c >= '0' && c <= '9') t = c - '0' + 52;
        if (c == '+') t = 62;
        if (c == '/') t = 63;
        if (c == '=') t = T_PAD;
        s_tab[c] = (uint8_t)t;
    }

    // ---------------------------------------------------------------- features
    const Field ff = field_of(a, d, F_FEATS, O * F * 4);
    if (ff.dead) flag |= BAD_LEN | (1u << (8 + F_FEATS));
    const int units = (ff.bytes + UNIT_BYTES - 1) / UNIT_BYTES, slabs = (units + NT - 1) / NT;
    const int sh = (int)(ff.off & 15), sd = sh >> 2, sb = sh & 3;
    const int64_t word0 = ff.off >> 4;                   // the aligned word that holds the field's first character
    const int64_t end_word = (ff.off + 4 * (int64_t)ff.quads + 15) >> 4;  // no word from here on holds one of its characters
    uint8_t* frow = a.feats ? (uint8_t*)a.feats + row * (int64_t)O * F * (BF16 ? 2 : 4) : nullptr;

    u4 raw[8], extra = {0u, 0u, 0u, 0u};
    auto fetch = [&](int s) {
        const int64_t w = word0 + (int64_t)s * (NT * 8) + tid;
#pragma unroll
        for (int k = 0; k < 8; ++k) raw[k] = !ff.dead && w + k * NT < end_word ? load_word(a, w + k * NT) : (u4){0u, 0u, 0u, 0u};
        // the word behind the slab: the tail of its last unit when the field does not start on a word
        if (tid == 0) extra = !ff.dead && w + 8 * NT < end_word ? load_word(a, w + 8 * NT) : (u4){0u, 0u, 0u, 0u};
    };
    fetch(0);
    for (int s = 0; s < slabs; ++s) {
        // word i = k NT + tid of the slab is place i % 8 of unit i / 8, and place 8 of the unit before when i % 8 == 0
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = k * NT + tid;
            *reinterpret_cast<u4*>(s_text + (i >> 3) * UNIT_STRIDE + (i & 7) * 16) = raw[k];
            if ((i & 7) == 0 && i > 0) *reinterpret_cast<u4*>(s_text + ((i >> 3) - 1) * UNIT_STRIDE + 128) = raw[k];
        }
        if (tid == 0) *reinterpret_cast<u4*>(s_text + (NT - 1) * UNIT_STRIDE + 128) = extra;
        __syncthreads();
        if (s + 1 < slabs) fetch(s + 1);

        const int u = s * NT + tid;
        if (u < units) {  // also without a feats table: the field's flags do not depend on which outputs are asked for
            const int ob = min(UNIT_BYTES, ff.bytes - u * UNIT_BYTES);  // a multiple of 32: F % 8 == 0
            uint32_t D[24];
            u4 lo = *reinterpret_cast<const u4*>(s_text + tid * UNIT_STRIDE);
#pragma unroll
            for (int g = 0; g < 8; ++g) {  // 16 characters, byte-aligned out of two words -> four quads -> three dwords
                const u4 hi = *reinterpret_cast<const u4*>(s_text + tid * UNIT_STRIDE + g * 16 + 16);
                const uint32_t A[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                lo = hi;
                uint32_t B[5], c[4];
#pragma unroll
                for (int j = 0; j < 5; ++j) B[j] = sd == 0 ? A[j] : sd == 1 ? A[j + 1] : sd == 2 ? A[j + 2] : A[j + 3];
#pragma unroll
                for (int j = 0; j < 4; ++j) c[j] = __builtin_amdgcn_alignbyte(B[j + 1], B[j], sb);
                uint32_t x[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int Q = u * 32 + g * 4 + q;  // the quad's index in the field
                    bool bad;
                    x[q] = quad_bytes(s_tab[c[q] & 255u], s_tab[(c[q] >> 8) & 255u], s_tab[(c[q] >> 16) & 255u], s_tab[c[q] >> 24],
                                      Q == ff.quads - 1 ? ff.pad : 0, bad);
                    if (Q >= ff.quads || ff.dead) {
                        x[q] = 0u;
                    } else if (bad) {
                        flag |= BAD_CHAR | (1u << (8 + F_FEATS));
                    }
                }
                D[3 * g] = x[0] | x[1] << 24;
                D[3 * g + 1] = x[1] >> 8 | x[2] << 16;
                D[3 * g + 2] = x[2] >> 16 | x[3] << 8;
            }
#pragma unroll
            for (int j = 0; j < 24; ++j)
                if (4 * j < ob && (D[j] & 0x7F800000u) == 0x7F800000u) flag |= NONFINITE;
            if (BF16) {
                uint8_t* dst = frow + (int64_t)u * (UNIT_BYTES / 2);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    u4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = bf16_rne(D[8 * k + 2 * j]) | (uint32_t)bf16_rne(D[8 * k + 2 * j + 1]) << 16;
                    if (frow && 32 * k + 32 <= ob) *reinterpret_cast<u4*>(dst + 16 * k) = o;
                }
            } else {
                uint8_t* dst = frow + (int64_t)u * UNIT_BYTES;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (frow && 16 * k + 16 <= ob) *reinterpret_cast<u4*>(dst + 16 * k) = (u4){D[4 * k], D[4 * k + 1], D[4 * k + 2], D[4 * k + 3]};
            }
        }
        __syncthreads();  // the next slab overwrites s_text
    }

    // ---------------------------------------------------------------- the five small fields, through LDS bytes
    // regions of s_text (O <= 128): ids 2 x 1024, confidences 2 x 512, boxes 2048
    constexpr int R_OBJ_ID = 0, R_ATTR_ID = 1024, R_OBJ_CONF = 2048, R_ATTR_CONF = 2560, R_BOXES = 3072;
    auto small = [&](int f, int region, int bytes) -> bool {  // field f -> its bytes at s_text + region; true: dead
        const Field fd = field_of(a, d, f, bytes);
        if (fd.dead) {
            flag |= BAD_LEN | (1u << (8 + f));
            return true;
        }
        for (int q = tid; q < fd.quads; q += NT) {
            const uint8_t* c = a.text + fd.off + 4 * (int64_t)q;  // inside [off, off + len): len == 4 quads
            bool bad;
            const uint32_t x = quad_bytes(s_tab[c[0]], s_tab[c[1]], s_tab[c[2]], s_tab[c[3]], q == fd.quads - 1 ? fd.pad : 0, bad);
            if (bad) flag |= BAD_CHAR | (1u << (8 + f));
            uint8_t* o = s_text + region + 3 * q;
            o[0] = (uint8_t)x;  // the regions are exactly as large as their fields at O = 128: nothing behind the last byte
            if (3 * q + 1 < fd.bytes) o[1] = (uint8_t)(x >> 8);
            if (3 * q + 2 < fd.bytes) o[2] = (uint8_t)(x >> 16);
        }
        return false;
    };
    const bool dead_oid = small(F_OBJ_ID, R_OBJ_ID, 8 * O), dead_oc = small(F_OBJ_CONF, R_OBJ_CONF, 4 * O);
    const bool dead_aid = small(F_ATTR_ID, R_ATTR_ID, 8 * O), dead_ac = small(F_ATTR_CONF, R_ATTR_CONF, 4 * O);
    const bool dead_box = small(F_BOXES, R_BOXES, 16 * O);
    __syncthreads();
    const uint32_t* s_w = reinterpret_cast<const uint32_t*>(s_text);
    auto ids = [&](int32_t* out, int region, bool dead) {  // int64 -> int32
        if (!out || tid >= O) return;
        const uint32_t lo = s_w[region / 4 + 2 * tid], hi = s_w[region / 4 + 2 * tid + 1];
        const bool fits = hi == (uint32_t)((int32_t)lo >> 31);
        if (!dead && !fits) flag |= BAD_ID;
        out[row * O + tid] = dead || !fits ? 0 : (int32_t)lo;
    };
    ids(a.obj_labels, R_OBJ_ID, dead_oid);
    ids(a.attr_labels, R_ATTR_ID, dead_aid);
    if (a.obj_confs && tid < O) reinterpret_cast<uint32_t*>(a.obj_confs)[row * O + tid] = dead_oc ? 0u : s_w[R_OBJ_CONF / 4 + tid];
    if (a.attr_confs && tid < O) reinterpret_cast<uint32_t*>(a.attr_confs)[row * O + tid] = dead_ac ? 0u : s_w[R_ATTR_CONF / 4 + tid];
    if (a.boxes) {
        const float w = (float)d[2 * NF], h = (float)d[2 * NF + 1];
        for (int j = tid; j < 4 * O; j += NT) {
            float b = dead_box ? 0.f : __uint_as_float(s_w[R_BOXES / 4 + j]);
            if (a.normalize) b = __fdiv_rn(b, (j & 1) ? h : w);
            const double bd = (double)b;
            if (a.normalize && !dead_box && !(bd < 1.0 + 1e-5 && -bd < 1e-5)) flag |= BAD_BOX;
            a.boxes[row * O * 4 + j] = b;
        }
    }

    // the line's flag word: OR over the wave, then over the four waves through LDS; thread 0 owns the outputs
    __shared__ uint32_t s_flag[NT / 64];
    for (int o = 32; o; o >>= 1) flag |= (uint32_t)__shfl_xor((int)flag, o);
    if ((tid & 63) == 0) s_flag[tid >> 6] = flag;
    __syncthreads();
    if (tid == 0) {
        flag = s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3];
        if (a.flags) a.flags[line] = flag;
        if (a.counts) {
            if (flag & (BAD_CHAR | BAD_LEN | BAD_ID)) atomicAdd(a.counts, 1);
            if (flag & BAD_BOX) atomicAdd(a.counts + 1, 1);
        }
    }
}

bool aligned(const void* p, uintptr_t n) { return (uintptr_t)p % n == 0; }
}  // namespace

extern "C" int xggm_tsv_decode(const xggm_tsv_decode_args* args, hipStream_t st) {
    const char* who = "xggm_tsv_decode";
    XGGM_REQUIRE(args, "%s: null argument struct", who);
    const xggm_tsv_decode_args& a = *args;
    XGGM_REQUIRE(a.text && a.desc && a.host_desc, "%s: null text, desc (device) or host_desc (its host copy)", who);
    XGGM_REQUIRE(a.feats || a.boxes || a.obj_labels || a.attr_labels || a.obj_confs || a.attr_confs || a.flags || a.counts,
                 "%s: every output pointer is null", who);
    XGGM_REQUIRE(a.n >= 1 && a.n < (1ll << 31), "%s: n=%lld lines, [1, 2^31) expected", who, (long long)a.n);
    XGGM_REQUIRE(a.O >= 1 && a.O <= XGGM_TSV_MAX_OBJECTS, "%s: O=%d objects outside [1, %d]", who, a.O, XGGM_TSV_MAX_OBJECTS);
    XGGM_REQUIRE(a.F >= 1 && a.F % 8 == 0 && (int64_t)a.O * a.F < (1ll << 28),
                 "%s: F=%d must be a positive multiple of 8 (feature rows move 16 bytes per lane) with O F < 2^28", who, a.F);
    XGGM_REQUIRE(a.row0 >= 0 && a.capacity >= 0 && a.row0 <= a.capacity - a.n,
                 "%s: rows [%lld, %lld) leave the table's capacity of %lld rows", who, (long long)a.row0, (long long)(a.row0 + a.n),
                 (long long)a.capacity);
    XGGM_REQUIRE(a.n_bytes >= 0 && a.alloc_bytes >= a.n_bytes && a.alloc_bytes % 16 == 0 && aligned(a.text, 16),
                 "%s: the text buffer must be 16-byte aligned and its allocation (%lld bytes) a multiple of 16 that holds n_bytes=%lld",
                 who, (long long)a.alloc_bytes, (long long)a.n_bytes);
    XGGM_REQUIRE(aligned(a.desc, 8) && aligned(a.host_desc, 8), "%s: misaligned descriptor table (8 bytes)", who);
    XGGM_REQUIRE(aligned(a.feats, 16), "%s: feats is not 16-byte aligned", who);
    XGGM_REQUIRE(aligned(a.boxes, 4) && aligned(a.obj_labels, 4) && aligned(a.attr_labels, 4) && aligned(a.obj_confs, 4) &&
                     aligned(a.attr_confs, 4) && aligned(a.flags, 4) && aligned(a.counts, 4),
                 "%s: misaligned table (boxes, labels, confidences, flags, counts: 4 bytes)", who);
    for (int64_t i = 0; i < a.n; ++i) {
        const int64_t* d = a.host_desc + i * ND;
        for (int f = 0; f < NF; ++f) {
            const int64_t off = d[2 * f], len = d[2 * f + 1];
            XGGM_REQUIRE(off >= 0 && len >= 0, "%s: line %lld field %d has a negative offset or length (%lld, %lld)", who, (long long)i, f,
                         (long long)off, (long long)len);
            XGGM_REQUIRE(off <= a.n_bytes && len <= a.n_bytes - off, "%s: line %lld field %d [%lld, +%lld) ends past n_bytes=%lld", who,
                         (long long)i, f, (long long)off, (long long)len, (long long)a.n_bytes);
        }
        if (a.normalize)
            XGGM_REQUIRE(d[2 * NF] >= 1 && d[2 * NF] < (1 << 24) && d[2 * NF + 1] >= 1 && d[2 * NF + 1] < (1 << 24),
                         "%s: line %lld has img_w=%lld img_h=%lld outside [1, 2^24)", who, (long long)i, (long long)d[2 * NF],
                         (long long)d[2 * NF + 1]);
    }
    if (a.feats_bf16)
        hipLaunchKernelGGL(tsv_decode_kernel<true>, dim3((unsigned)a.n), dim3(NT), 0, st, a);
    else
        hipLaunchKernelGGL(tsv_decode_kernel<false>, dim3((unsigned)a.n), dim3(NT), 0, st, a);
    return xggm_check_launch(who);
}

/*
 * cstripe_gpu.hip — MI355X (gfx950/CDNA4) device path of the columnar scan:
 * HtoD staging of compressed chunk streams, LZ4 segment decode kernel, and
 * the fused predicate-filter + partial-aggregate kernels.
 *
 * This replaces, with HIP kernels, the CPU loops under ColumnarReadNextRow:
 *   - DecompressBuffer/LZ4_decompress_safe per chunk
 *     (columnar_compression.c:165-198)           -> lz4_decode_kernel
 *   - DeserializeBoolArray (columnar_reader.c:1506-1534): exists bitmaps are
 *     NOT unpacked — kernels consume the packed bits directly (rank tables
 *     precomputed host-side at stage)
 *   - DeserializeDatumArray (columnar_reader.c:1542-1572): fixed-width value
 *     streams are read as coalesced typed loads (layout guaranteed by
 *     SerializeSingleDatum, columnar_writer.c:555-585)
 *   - per-row qual eval (ExecQual under columnar_customscan.c:1907-1913)
 *     -> predicate evaluation in-register, per 64-lane wavefront
 *   - PG Agg transition + worker_partial_agg (aggregate_utils.c:501-607)
 *     -> per-thread accumulate, wave shuffle reduce, LDS cross-wave reduce,
 *        per-block partial, device-wide final reduce (no global atomics)
 *
 * All scan/filter/reduce — HBM-bandwidth bound; no MFMA (north star).
 * Wavefront = 64 throughout; __ballot is 64-bit.
 */
#include "internal.h"
#include "compress.h"
#include "pglz.h"
#include "zstd_r.h"
#include "lz4_enc.h"
#include "vartext.h"
#include "like.h"

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>
#include <cstdio>
#include <vector>
#include <algorithm>

#define WAVE 64
#define AGG_BLOCK 256
#define TILE_ROWS 4096
#define MAX_PREDS CSTRIPE_MAX_PREDS
#define MAX_AGGS 12
#define MAX_PROJ 16

/* ---------------- device-side descriptors ---------------- */

struct SegDesc {
    uint64_t src_off;       /* into d_data (compressed) */
    uint64_t dst_off;       /* into d_scratch (decompressed) */
    uint32_t comp_len;
    uint32_t decomp_len;
};

struct ColLoc {
    uint64_t val_off;       /* into d_scratch if (flags&1) else d_data */
    uint64_t exists_off;    /* into d_data (packed bitmap, 8B-padded) */
    uint32_t rank_off;      /* u32 word-rank table index into d_rank */
    uint16_t flags;         /* 1 = values in scratch; 2 = dense (no nulls);
                             * 4 = canonical stream (closed-form access) */
    uint8_t  type;          /* cstripe_type */
    uint8_t  width;
    /* canonical-stream chunks (flags & 4): value bytes are read closed-form
     * straight from the staged COMPRESSED stream at val_off (format.h) */
    int64_t  hval;          /* P: shared high bytes, already in place;
                             * CONST: the value; LIT: literal-run header len */
    uint8_t  mode;          /* CSF_SEGMODE_* */
    uint8_t  L;             /* P(L): varying low bytes per value */
    uint8_t  pad[6];
};

struct GroupDesc {
    uint32_t row_count;
    uint32_t colbase;       /* index into d_colloc: colbase + proj_idx */
};

struct PredD {
    uint16_t proj;
    uint8_t  op;
    uint8_t  is_float;
    uint8_t  gend;       /* 1 = last member of its OR group (groups are
                          * contiguous; pass &= OR of the group's members) */
    uint8_t  pad[7];
    int64_t  ival;
    double   fval;
};

struct AggD {
    uint8_t kind;
    uint8_t proj_a, proj_b, proj_c;
    int64_t one;
};

struct AggParams {
    uint32_t n_preds, n_aggs, n_proj, tiles_per_group, n_groups;
    uint32_t pad[3];
    PredD preds[MAX_PREDS];
    AggD aggs[MAX_AGGS];
};

struct FusedTile;

/* per-block / final accumulator cell (32 B) */
struct AccCell {
    int64_t lo;             /* i128 low  / i64 min-max */
    int64_t hi;             /* i128 high */
    double  f;              /* f64 sum / min / max */
    int64_t cnt;            /* contributing rows */
};

struct cs_gpu_state {
    int device = -1;
    hipStream_t stream = nullptr;
    uint8_t *d_data = nullptr;       /* staged compressed values + exists */
    uint8_t *d_scratch = nullptr;    /* decompressed value streams */
    uint32_t *d_rank = nullptr;
    SegDesc *d_segs = nullptr;
    GroupDesc *d_groups = nullptr;
    ColLoc *d_colloc = nullptr;
    AccCell *d_block = nullptr;
    AccCell *d_final = nullptr;
    AccCell *d_final2 = nullptr;     /* wide-pass outputs of the final reduce */
    uint32_t *d_gkeys = nullptr;     /* grouped: per-block key tables */
    AccCell *d_gcells = nullptr;
    uint32_t *d_gfkeys = nullptr;    /* grouped: final merged groups */
    AccCell *d_gfcells = nullptr;
    uint32_t *d_gn = nullptr;
    uint8_t *d_tmp = nullptr;        /* next_batch: canonical-chunk decode buf */
    uint64_t tmp_bytes = 0;
    bool batch_decoded = false;      /* scratch holds decoded streams */
    SegDesc *d_zsegs = nullptr;      /* restricted-zstd segments (zstd_r.h) */
    uint32_t n_zsegs = 0;
    uint32_t max_zseg_comp = 0;      /* largest zstd frame (LDS-variant gate) */
    uint32_t max_zseg_dlen = 0;      /* largest zstd frame decompressed */
    zr_dtables *d_zrtab = nullptr;   /* predefined FSE decode tables */
    std::vector<uint8_t> col_scratch;/* per proj: any chunk lands in scratch */
    bool any_zr = false;             /* some staged stream is zstd canonical */
    std::vector<uint8_t> col_ov;     /* per proj: every selected chunk group
                                      * holds it dense I64 canonical P(L) or
                                      * CONST (multi_agg_kernel_ov's shapes) */
    int n_cus = 0;                   /* compute units, sizes the fixed grids */
    uint32_t max_group_rows = 0;     /* largest selected chunk group */
    int *d_error = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    /* scan_select (filtered row materialisation): per-tile pass masks,
     * counts and output bases, cached once computed — predicates are fixed
     * at scan_begin, so only scan_end / restage drops them */
    uint64_t *d_sel_mask = nullptr;     /* [tiles][64] pass words, 1 bit/row */
    uint32_t *d_sel_counts = nullptr;   /* [tiles] passing rows */
    uint64_t *d_sel_bases = nullptr;    /* [tiles] exclusive scan of counts */
    uint64_t *d_sel_total = nullptr;    /* one word: rows that passed */
    uint64_t *d_sel_rowbase = nullptr;  /* [groups] table-wide first row */
    uint8_t *d_sel_out = nullptr;       /* host-mode compaction buffer */
    uint64_t sel_out_bytes = 0;
    bool sel_cached = false;
    uint64_t sel_total = 0;
    hipEvent_t sev[4] = {nullptr, nullptr, nullptr, nullptr};
    /* scan_agg_hashed: open-addressing table (key words + accumulator
     * cells), the dense compaction target and its counter; grown when
     * capacity or n_aggs needs it */
    unsigned long long *d_hkeys = nullptr;     /* [slots] packed keys / EMPTY */
    struct ThreadAcc *d_hcells = nullptr;      /* [slots * n_aggs] */
    unsigned long long *d_hokeys = nullptr;    /* [capacity] compacted keys */
    AccCell *d_hocells = nullptr;              /* [capacity * n_aggs] */
    unsigned long long *d_hcount = nullptr;    /* one word: occupied slots */
    uint64_t hkeys_slots = 0, hcells_n = 0, hokeys_n = 0, hocells_n = 0;
    hipEvent_t hev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    /* scan_agg_hashed_topn: indices of the groups HAVING kept, their order
     * and tie words, the state block, two radix-select states (order word,
     * tie word) and the limit-sized gather buffer. Grow-only. */
    uint32_t *d_gt_kept = nullptr;      /* [capacity] indices into d_hokeys */
    uint64_t *d_gt_ord = nullptr;       /* [capacity] order word per kept group */
    uint64_t *d_gt_tie = nullptr;       /* [capacity] tie word per kept group */
    struct GtopnState *d_gt_state = nullptr;
    struct TopnState *d_gt_sel = nullptr;   /* [2] */
    uint8_t *d_gt_out = nullptr;        /* limit * (24 + 32 * n_aggs) bytes */
    uint64_t gt_kept_n = 0, gt_ord_n = 0, gt_tie_n = 0, gt_out_bytes = 0;
    hipEvent_t gev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    /* scan_select_topn: the compact key array (8 B per passing row), the
     * radix-select state block, and the refined mask / counts / bases — its
     * own buffers, the d_sel_* cache above is only ever read. Grow-only. */
    uint64_t *d_tn_keys = nullptr;      /* [n_pass] packed keys, scan order */
    uint64_t *d_tn_okeys = nullptr;     /* [limit] keys of the emitted rows */
    struct TopnState *d_tn_state = nullptr;
    uint64_t *d_tn_mask = nullptr;      /* [tiles][64] key < T, then final */
    uint64_t *d_tn_eq = nullptr;        /* [tiles][64] key == T */
    uint32_t *d_tn_counts = nullptr;    /* [tiles] tie counts, then final */
    uint64_t *d_tn_tbases = nullptr;    /* [tiles] exclusive scan of ties */
    uint64_t *d_tn_bases = nullptr;     /* [tiles] exclusive scan of final */
    uint64_t *d_tn_total = nullptr;     /* [2] ties on T, rows emitted */
    uint8_t *d_tn_emit = nullptr;       /* scan-order rows before the permute */
    uint8_t *d_tn_out = nullptr;        /* host-mode permuted staging */
    uint32_t *d_tn_perm = nullptr;      /* [limit] final order -> scan order */
    uint64_t tn_keys_n = 0, tn_okeys_n = 0, tn_mask_n = 0, tn_eq_n = 0,
             tn_counts_n = 0, tn_tbases_n = 0, tn_bases_n = 0,
             tn_emit_bytes = 0, tn_out_bytes = 0, tn_perm_n = 0;
    hipEvent_t tev[8] = {nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr};

    uint64_t data_bytes = 0;
    uint64_t scratch_bytes = 0;
    uint32_t n_segs = 0;
    uint32_t max_seg_comp = 0;
    uint32_t max_seg_dlen = 0;
    bool segs_16aligned = true;
    bool fusable = true;             /* all proj cols dense i64, uniform 256B lz4 segs */
    bool all_dense = true;           /* no NULLs anywhere -> pair_agg_kernel */
    struct FusedTile *d_tiles = nullptr;
    uint32_t n_tiles = 0;
    uint32_t n_groups = 0;
    uint32_t n_proj = 0;
    uint32_t max_blocks = 0;
    int proj_of_col[64];             /* column index -> projected slot (-1) */
    uint8_t proj_type[MAX_PROJ];
    /* host-side mirror for next_batch (exists read from mmap) */
    std::vector<uint64_t> scratch_off;  /* per (sel,proj): decomp offset */
    std::vector<ColLoc> colloc_host;
    /* VARTEXT predicates translated at stage into integer atoms over the
     * column's dictionary ranks, parallel to scan->preds (fill_preds) */
    std::vector<uint8_t> tpred_op;
    std::vector<int64_t> tpred_ival;
    /* IN / NOT IN: one member slot (a projected I8 membership column in
     * scratch, after the table columns) per distinct (column, set) pair;
     * mpred_slot is parallel to scan->preds, -1 for every other predicate */
    struct MemberSlot { uint32_t col, set, proj; bool like; };
    std::vector<MemberSlot> mslots;
    std::vector<int> mpred_slot;
    /* LIKE / NOT LIKE: a member slot too, one per distinct (column, pattern
     * bytes) pair — `like` set, `set` the index of a text constant holding
     * the pattern; filled by vartext_build, skipped by sets_build.
     * like_form[table column] is the CSTRIPE_LIKE_FORM_* of this stage. */
    std::vector<uint8_t> like_form;
    std::vector<void *> set_bufs;    /* set and lookup tables (sets_build,
                                      * lookups_build) */
    /* lookups: one derived slot (a projected sparse I64 column in scratch,
     * after the member slots) per payload; proj_of_col covers their ids */
    struct DerivedSlot { uint32_t lookup, payload, proj; };
    std::vector<DerivedSlot> dslots;
    /* expressions: one computed slot (a projected sparse I64 column in
     * scratch, after the derived slots) per expression */
    std::vector<uint32_t> eslots;    /* [expression] -> projected slot */
};

/* ---------------- error helper ---------------- */

#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) { \
    cs_set_err("%s failed: %s", #x, hipGetErrorString(_e)); return CSTRIPE_ERR; } } while (0)

extern "C" int cstripe_gpu_available(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n > 0 ? 1 : 0;
}

/* =====================================================================
 * LZ4 block decode — one 64-lane wavefront per independently decodable
 * segment. All lanes parse the sequence header redundantly (same-address
 * loads broadcast); literal and match copies are lane-parallel. Overlapping
 * matches (offset < length) resolve every byte to the pre-existing pattern
 * window via modulo, so one parallel pass is race-free.
 * Implements the LZ4 block format consumed by LZ4_decompress_safe
 * (columnar_compression.c:183); any valid block decodes, segmented or not.
 *
 * Two variants:
 *  - lz4_decode_lds_kernel: compressed segment is first staged into LDS with
 *    coalesced u32 loads and the OUTPUT is decoded in LDS too, so the
 *    byte-serial parse and all match copies run at LDS latency instead of
 *    chained dependent HBM round trips; the finished segment is flushed to
 *    global with coalesced 16 B stores. Needs in+out <= 64 KiB of LDS —
 *    the writer's default 8 KiB segments give ~9 resident waves/CU.
 *  - lz4_decode_kernel: the global-memory fallback for oversized segments
 *    (e.g. single-block whole-chunk compatibility mode).
 * ===================================================================== */

template <bool IN_LDS>
__device__ inline void lz4_body(const uint8_t *__restrict__ src, uint32_t slen,
                                uint8_t *__restrict__ dst, uint32_t dlen,
                                uint32_t lane, int *__restrict__ err)
{
    uint32_t ip = 0, op = 0;
    while (ip < slen) {
        const uint32_t token = src[ip++];
        /* literals */
        uint32_t litlen = token >> 4;
        if (litlen == 15) {
            uint32_t b;
            do { b = src[ip++]; litlen += b; } while (b == 255 && ip < slen);
        }
        if (ip + litlen > slen || op + litlen > dlen) { if (lane == 0) atomicOr(err, 1); return; }
        for (uint32_t j = lane; j < litlen; j += WAVE) dst[op + j] = src[ip + j];
        ip += litlen;
        op += litlen;
        if (ip >= slen) break;           /* last sequence: literals only */

        /* match */
        if (ip + 2 > slen) { if (lane == 0) atomicOr(err, 1); return; }
        uint32_t offset = (uint32_t)src[ip] | ((uint32_t)src[ip + 1] << 8);
        ip += 2;
        uint32_t mlen = token & 15;
        if (mlen == 15) {
            uint32_t b;
            do { b = src[ip++]; mlen += b; } while (b == 255 && ip < slen);
        }
        mlen += 4;
        if (offset == 0 || offset > op || op + mlen > dlen) { if (lane == 0) atomicOr(err, 1); return; }
        const uint32_t mstart = op - offset;
        if (offset >= mlen) {
            for (uint32_t j = lane; j < mlen; j += WAVE) dst[op + j] = dst[mstart + j];
        } else {
            /* every byte's ultimate source lies in the pre-existing pattern
             * window [op-offset, op) — single race-free parallel pass */
            for (uint32_t j = lane; j < mlen; j += WAVE) dst[op + j] = dst[mstart + (j % offset)];
        }
        op += mlen;
    }
    if (op != dlen) { if (lane == 0) atomicOr(err, 2); }
}

__global__ __launch_bounds__(WAVE) void lz4_decode_kernel(
    const uint8_t *__restrict__ data, uint8_t *__restrict__ scratch,
    const SegDesc *__restrict__ segs, int *__restrict__ err)
{
    const SegDesc s = segs[blockIdx.x];
    lz4_body<false>(data + s.src_off, s.comp_len, scratch + s.dst_off,
                    s.decomp_len, threadIdx.x, err);
}

/* =====================================================================
 * Lane-parallel LZ4 decode — ONE LANE per micro-segment (writer default
 * 512 B decompressed). Why: this data compresses to ~one sequence per
 * 8-byte value (measured ~8 B/sequence), so a wave-cooperative decoder is
 * serialized on the per-sequence parse chain and moves ~8 B per chain step.
 * Here every wave advances 64 independent segment streams per step:
 *  - input: per-lane 16-byte register window over the compressed stream,
 *    refilled with aligned u64 loads (one dependent global load per 8
 *    compressed bytes instead of per byte)
 *  - output: per-lane LDS region (stride 528 = 16-byte aligned, 4-bank
 *    skew per lane so equal-progress lanes hit different banks); match
 *    copies are plain per-lane sequential byte moves (memmove-forward
 *    semantics handles overlap for free)
 *  - finish: block-cooperative 16 B coalesced flush LDS -> scratch
 * ===================================================================== */

struct ByteStream {
    const uint8_t *base;    /* 8B-aligned */
    uint64_t w0, w1, w2, w3; /* 32-byte window; ~24 B of refill lookahead */
    uint32_t woff;          /* byte offset of w0 within base */
    uint32_t pos;           /* current byte position (>= initial shift) */
};

__device__ inline void bs_init(ByteStream &b, const uint8_t *data, uint64_t off)
{
    uint64_t a = off & ~15ull;           /* 16B-aligned base */
    b.base = data + a;
    b.pos = (uint32_t)(off - a);
    b.woff = 0;
    b.w0 = *(const uint64_t *)(b.base);
    b.w1 = *(const uint64_t *)(b.base + 8);
    b.w2 = *(const uint64_t *)(b.base + 16);
    b.w3 = *(const uint64_t *)(b.base + 24);
}

__device__ inline void bs_norm(ByteStream &b)
{
    while (b.pos - b.woff >= 8) {
        b.w0 = b.w1;
        b.w1 = b.w2;
        b.w2 = b.w3;
        b.woff += 8;
        b.w3 = *(const uint64_t *)(b.base + b.woff + 24);
    }
}

__device__ inline uint8_t bs_get(ByteStream &b)
{
    bs_norm(b);
    uint32_t rel = b.pos - b.woff;
    b.pos++;
    return (uint8_t)(b.w0 >> (8 * rel));
}

/* next 8 bytes at pos as a little-endian u64 (rel in [0,8) after bs_norm) */
__device__ inline uint64_t bs_peek64(ByteStream &b)
{
    bs_norm(b);
    uint32_t s = 8 * (b.pos - b.woff);
    return s ? ((b.w0 >> s) | (b.w1 << (64 - s))) : b.w0;
}

/* decode ONE segment, per-lane serial, output to this lane's LDS region.
 * Shared by the standalone decode kernel and the fused decode+agg kernel. */
__device__ inline void lz4_lane_decode(const uint8_t *__restrict__ data,
                                       const SegDesc &s, uint8_t *__restrict__ sout,
                                       int *__restrict__ err)
{
    {
        ByteStream bs;
        bs_init(bs, data, s.src_off);
        const uint32_t send = bs.pos + s.comp_len;   /* end position */
        const uint32_t dlen = s.decomp_len;
        uint32_t op = 0;
        bool bad = false;
        while (bs.pos < send) {
            const uint32_t token = bs_get(bs);
            uint32_t litlen = token >> 4;
            if (litlen == 15) {
                uint32_t b;
                do { b = bs_get(bs); litlen += b; } while (b == 255 && bs.pos < send);
            }
            if (bs.pos + litlen > send || op + litlen > dlen) { bad = true; break; }
            {   /* literal copy: 8 bytes per window peek, then byte tail */
                uint32_t left = litlen;
                while (left >= 8) {
                    uint64_t v = bs_peek64(bs);
                    bs.pos += 8;
                    sout[op + 0] = (uint8_t)v;       sout[op + 1] = (uint8_t)(v >> 8);
                    sout[op + 2] = (uint8_t)(v >> 16); sout[op + 3] = (uint8_t)(v >> 24);
                    sout[op + 4] = (uint8_t)(v >> 32); sout[op + 5] = (uint8_t)(v >> 40);
                    sout[op + 6] = (uint8_t)(v >> 48); sout[op + 7] = (uint8_t)(v >> 56);
                    op += 8;
                    left -= 8;
                }
                for (uint32_t j = 0; j < left; j++) sout[op + j] = bs_get(bs);
                op += left;
            }
            if (bs.pos >= send) break;       /* last sequence: literals only */

            if (bs.pos + 2 > send) { bad = true; break; }
            uint32_t offset = (uint32_t)bs_get(bs);
            offset |= (uint32_t)bs_get(bs) << 8;
            uint32_t mlen = token & 15;
            if (mlen == 15) {
                uint32_t b;
                do { b = bs_get(bs); mlen += b; } while (b == 255 && bs.pos < send);
            }
            mlen += 4;
            if (offset == 0 || offset > op || op + mlen > dlen) { bad = true; break; }
            /* uniform per-lane byte copy — control flow stays convergent
             * across the wave (a branchier word-copy variant measured 2x the
             * per-byte instructions from divergence; profiles/r01).
             * 4-wide manual unroll: the 4 loads are independent and issue
             * together instead of load-wait-store per byte. Overlap safety:
             * offset<4 would make loads of a quad depend on its own stores,
             * so quads only when offset>=4; sources are then complete. */
            const uint8_t *msrc = sout + op - offset;
            uint32_t j = 0;
            if (((offset | op) & 3) == 0) {
                /* word-granular stream (e.g. the 4-byte varlena slots of
                 * text columns): source, destination and offset are all
                 * 4-aligned, so copies run as aligned LDS words — the
                 * u32-splat case (offset 4: one repeated slot) is the
                 * dominant shape of low-cardinality flag columns */
                uint32_t *d32 = (uint32_t *)(sout + op);
                if (offset == 4) {
                    const uint32_t v = *(const uint32_t *)msrc;
                    for (; j + 4 <= mlen; j += 4) d32[j >> 2] = v;
                } else {
                    const uint32_t *s32 = (const uint32_t *)msrc;
                    const uint32_t woff = offset >> 2;
                    for (; j + 4 <= mlen; j += 4) {
                        /* overlap-safe: reads trail writes by woff words */
                        d32[j >> 2] = (j >> 2) < woff ? s32[j >> 2]
                                                      : d32[(j >> 2) - woff];
                    }
                }
            } else if (offset >= 8) {
                for (; j + 8 <= mlen; j += 8) {
                    uint8_t b0 = msrc[j], b1 = msrc[j + 1];
                    uint8_t b2 = msrc[j + 2], b3 = msrc[j + 3];
                    uint8_t b4 = msrc[j + 4], b5 = msrc[j + 5];
                    uint8_t b6 = msrc[j + 6], b7 = msrc[j + 7];
                    sout[op + j] = b0; sout[op + j + 1] = b1;
                    sout[op + j + 2] = b2; sout[op + j + 3] = b3;
                    sout[op + j + 4] = b4; sout[op + j + 5] = b5;
                    sout[op + j + 6] = b6; sout[op + j + 7] = b7;
                }
            } else if (offset >= 4) {
                for (; j + 4 <= mlen; j += 4) {
                    uint8_t b0 = msrc[j], b1 = msrc[j + 1];
                    uint8_t b2 = msrc[j + 2], b3 = msrc[j + 3];
                    sout[op + j] = b0; sout[op + j + 1] = b1;
                    sout[op + j + 2] = b2; sout[op + j + 3] = b3;
                }
            }
            for (; j < mlen; j++) sout[op + j] = msrc[j];
            op += mlen;
        }
        if (bad || op != dlen) atomicOr(err, 4);
    }
}

__global__ void lz4_decode_lane_kernel(
    const uint8_t *__restrict__ data, uint8_t *__restrict__ scratch,
    const SegDesc *__restrict__ segs, uint32_t n_segs, uint32_t stride,
    int *__restrict__ err)
{
    extern __shared__ uint8_t sout_all[];
    const uint32_t tid = threadIdx.x;
    const uint32_t first = blockIdx.x * blockDim.x;
    const uint32_t gseg = first + tid;
    uint8_t *sout = sout_all + (size_t)tid * stride;
    /* per-segment (dst_off, decomp_len) cached in LDS for the flush loop */
    uint64_t *sdst = (uint64_t *)(sout_all + (size_t)blockDim.x * stride);
    uint32_t *sdlen = (uint32_t *)(sdst + blockDim.x);

    if (gseg < n_segs) {
        const SegDesc s = segs[gseg];
        sdst[tid] = s.dst_off;
        sdlen[tid] = s.decomp_len;
        lz4_lane_decode(data, s, sout, err);
    }
    __syncthreads();

    /* cooperative coalesced flush: 16 B global stores (full coalescing)
     * assembled from four 4 B LDS reads — the region stride is a 4-mod-8
     * multiple so the decode loop's byte ops are bank-conflict-free, which
     * makes LDS-side 16 B alignment unavailable */
    const uint32_t eps = (stride + 15) >> 4;          /* 16B slots per segment */
    const uint32_t in_block = min(blockDim.x, n_segs - first);
    const uint32_t total = in_block * eps;
    for (uint32_t f = tid; f < total; f += blockDim.x) {
        const uint32_t sidx = f / eps;
        const uint32_t boff = (f % eps) << 4;
        const uint32_t dl = sdlen[sidx];
        if (boff >= dl) continue;
        uint8_t *dst = scratch + sdst[sidx] + boff;
        const uint32_t *ls = (const uint32_t *)(sout_all + (size_t)sidx * stride + boff);
        if (boff + 16 <= dl) {
            uint4 v;
            v.x = ls[0]; v.y = ls[1]; v.z = ls[2]; v.w = ls[3];
            *(uint4 *)dst = v;                        /* dst 16B-aligned (writer) */
        } else {
            const uint8_t *lb = (const uint8_t *)ls;
            for (uint32_t j = 0; j < dl - boff; j++) dst[j] = lb[j];
        }
    }
}

__global__ __launch_bounds__(WAVE) void lz4_decode_lds_kernel(
    const uint8_t *__restrict__ data, uint8_t *__restrict__ scratch,
    const SegDesc *__restrict__ segs, uint32_t in_cap, int *__restrict__ err)
{
    extern __shared__ uint8_t sbuf[];      /* [in_cap compressed][output] */
    const SegDesc s = segs[blockIdx.x];
    const uint32_t lane = threadIdx.x;

    /* stage compressed bytes: aligned u32 loads from (src_off & ~3) */
    const uint64_t base = s.src_off & ~3ull;
    const uint32_t shift = (uint32_t)(s.src_off - base);
    const uint32_t words = (s.comp_len + shift + 3) >> 2;
    const uint32_t *gsrc = (const uint32_t *)(data + base);
    uint32_t *lin = (uint32_t *)sbuf;
    for (uint32_t j = lane; j < words; j += WAVE) lin[j] = gsrc[j];
    __syncthreads();

    uint8_t *out = sbuf + in_cap;
    lz4_body<true>(sbuf + shift, s.comp_len, out, s.decomp_len, lane, err);
    __syncthreads();

    /* coalesced flush LDS -> global */
    uint8_t *dst = scratch + s.dst_off;
    const uint32_t dlen = s.decomp_len;
    if (((uintptr_t)dst & 15) == 0) {
        uint32_t vec = dlen >> 4;
        uint4 *d4 = (uint4 *)dst;
        const uint4 *o4 = (const uint4 *)out;
        for (uint32_t j = lane; j < vec; j += WAVE) d4[j] = o4[j];
        for (uint32_t j = (vec << 4) + lane; j < dlen; j += WAVE) dst[j] = out[j];
    } else {
        for (uint32_t j = lane; j < dlen; j += WAVE) dst[j] = out[j];
    }
}

/* =====================================================================
 * Fused filter + partial aggregate (generic, ungrouped)
 * grid: n_groups * tiles_per_group blocks of AGG_BLOCK threads.
 * Each thread strides rows of its tile; per-thread register accumulators;
 * wave __shfl_down reduce; LDS cross-wave reduce; one AccCell per block.
 * ===================================================================== */

/* canonical-stream byte position of value j's low-L bytes, by mode family:
 * lz4 P(L) interleaves them with match tokens (csf_canon_p_pos); the
 * restricted-zstd P(L) frame holds them densely in its literal section
 * (csf_canon_zrp_pos) */
__device__ inline uint32_t canon_pos(uint8_t mode, uint32_t L, uint32_t j)
{
    if ((mode & 0xF0u) == CSF_SEGMODE_ZRP_BASE)
        return j == 0 ? 15u : 23u + (j - 1u) * L;
    const uint32_t pos = j * (L + 3u) + (6u - L);
    return j == 0 ? 1u : (j == 1 ? 9u : pos);
}

__device__ inline bool col_value(const uint8_t *__restrict__ data,
                                 const uint8_t *__restrict__ scratch,
                                 const uint32_t *__restrict__ rank,
                                 const ColLoc &cl, uint32_t row,
                                 int64_t &iv, double &fv)
{
    uint32_t idx = row;
    if (!(cl.flags & 2)) {   /* sparse: null check + rank indirection */
        const uint64_t *bm = (const uint64_t *)(data + cl.exists_off);
        uint64_t w = bm[row >> 6];
        uint64_t bit = 1ull << (row & 63);
        if (!(w & bit)) return false;
        idx = rank[cl.rank_off + (row >> 6)] + (uint32_t)__popcll(w & (bit - 1));
    }
    const uint8_t *base = (cl.flags & 1) ? scratch + cl.val_off : data + cl.val_off;
    if (cl.flags & 4) {
        /* canonical stream: value bytes at a CLOSED-FORM position in the
         * compressed stream — no LZ4 sequence parse, no scratch (format.h).
         * One unaligned dwordx2 load per value; consecutive rows sit
         * (L+3) bytes apart, so a wave's loads coalesce into a few lines. */
        if (cl.mode == CSF_SEGMODE_LIT) {
            base += (uint64_t)cl.hval;           /* skip literal-run header */
        } else if ((cl.mode & 0xF8u) == CSF_SEGMODE_ZR4B_BASE) {
            /* width-4 single-varying-byte / const slots (char(1) flags) */
            uint32_t slot = (uint32_t)cl.hval;
            if (cl.mode != CSF_SEGMODE_ZR4_CONST) {
                const uint32_t kk = cl.L;
                const uint32_t pos = 15u + (idx == 0 ? kk : idx + 3u + kk);
                slot |= (uint32_t)base[pos] << (8u * kk);
            }
            if (cl.type == CSTRIPE_F32) {
                float ff;
                __builtin_memcpy(&ff, &slot, 4);
                fv = ff;
                iv = 0;
            } else {
                iv = cl.type == CSTRIPE_TEXT ? (int64_t)slot : (int64_t)(int32_t)slot;
                fv = cl.type == CSTRIPE_TEXT ? 0.0 : (double)iv;
            }
            return true;
        } else {
            uint64_t raw;
            if (cl.mode == CSF_SEGMODE_CONST || cl.mode == CSF_SEGMODE_ZR_CONST) {
                raw = (uint64_t)cl.hval;
            } else {                             /* P(L), lz4 or zstd layout */
                const uint32_t Lx = cl.L;
                const uint32_t pos = canon_pos(cl.mode, Lx, idx);
                uint64_t lo;
                __builtin_memcpy(&lo, base + pos, 8);
                const uint64_t m = (~0ull) >> ((8u - Lx) * 8u);
                raw = (lo & m) | (uint64_t)cl.hval;
            }
            if (cl.type == CSTRIPE_F64) {
                __builtin_memcpy(&fv, &raw, 8);
                iv = 0;
            } else {
                iv = (int64_t)raw;
                fv = (double)iv;
            }
            return true;
        }
    }
    switch (cl.type) {
        case CSTRIPE_I8:  iv = ((const int8_t  *)base)[idx]; fv = (double)iv; break;
        case CSTRIPE_I16: iv = ((const int16_t *)base)[idx]; fv = (double)iv; break;
        case CSTRIPE_I32: iv = ((const int32_t *)base)[idx]; fv = (double)iv; break;
        case CSTRIPE_I64: iv = ((const int64_t *)base)[idx]; fv = (double)iv; break;
        case CSTRIPE_F32: fv = ((const float  *)base)[idx]; iv = 0; break;
        case CSTRIPE_TEXT: iv = (int64_t)((const uint32_t *)base)[idx]; fv = 0; break;
        default:          fv = ((const double *)base)[idx]; iv = 0; break;
    }
    return true;
}

/* PG float ordering (float.c float8_cmp_internal): NaN sorts greater than
 * every non-NaN and equal to itself — predicate + MIN/MAX semantics must
 * match the reference's float8 operators, not IEEE compares */
__device__ inline int f64cmp_pg(double a, double b)
{
    if (a > b) return 1;
    if (a < b) return -1;
    if (a == b) return 0;
    const bool na = (a != a), nb = (b != b);
    if (na && nb) return 0;
    return na ? 1 : -1;
}

__device__ inline bool pred_eval(const PredD &p, int64_t iv, double fv)
{
    if (p.is_float) {
        const int c = f64cmp_pg(fv, p.fval);
        switch (p.op) {
            case CSTRIPE_PRED_LT: return c <  0;
            case CSTRIPE_PRED_LE: return c <= 0;
            case CSTRIPE_PRED_GT: return c >  0;
            case CSTRIPE_PRED_GE: return c >= 0;
            case CSTRIPE_PRED_EQ: return c == 0;
            default:              return c != 0;
        }
    }
    switch (p.op) {
        case CSTRIPE_PRED_LT: return iv <  p.ival;
        case CSTRIPE_PRED_LE: return iv <= p.ival;
        case CSTRIPE_PRED_GT: return iv >  p.ival;
        case CSTRIPE_PRED_GE: return iv >= p.ival;
        case CSTRIPE_PRED_EQ: return iv == p.ival;
        default:              return iv != p.ival;
    }
}

struct ThreadAcc {
    int64_t lo, hi;   /* i128 sum (lo unsigned semantics) / i64 minmax in lo */
    double  f;
    int64_t cnt;
};

__device__ inline void acc_init(ThreadAcc &a, uint8_t kind)
{
    a.lo = 0; a.hi = 0; a.f = 0.0; a.cnt = 0;
    switch (kind) {
        case CSTRIPE_AGG_MIN_I64: a.lo = INT64_MAX; break;
        case CSTRIPE_AGG_MAX_I64: a.lo = INT64_MIN; break;
        /* PG order: NaN is the greatest float, so NaN is MIN's identity
         * (min(NaN, x) = x; min over only-NaN rows correctly stays NaN) */
        case CSTRIPE_AGG_MIN_F64: a.f = NAN; break;
        case CSTRIPE_AGG_MAX_F64: a.f = -INFINITY; break;
        default: break;
    }
}

__device__ inline void acc_add_i128(ThreadAcc &a, __int128 v)
{
    __int128 x = ((__int128)a.hi << 64) | (unsigned long long)a.lo;
    x += v;
    a.lo = (int64_t)(uint64_t)x;
    a.hi = (int64_t)(x >> 64);
}

__device__ inline void acc_merge(ThreadAcc &a, const ThreadAcc &b, uint8_t kind)
{
    switch (kind) {
        case CSTRIPE_AGG_MIN_I64: a.lo = min(a.lo, b.lo); break;
        case CSTRIPE_AGG_MAX_I64: a.lo = max(a.lo, b.lo); break;
        case CSTRIPE_AGG_MIN_F64: if (f64cmp_pg(b.f, a.f) < 0) a.f = b.f; break;
        case CSTRIPE_AGG_MAX_F64: if (f64cmp_pg(b.f, a.f) > 0) a.f = b.f; break;
        case CSTRIPE_AGG_SUM_F64: a.f += b.f; break;
        default: {  /* counts + i128 sums */
            unsigned long long lo = (unsigned long long)a.lo + (unsigned long long)b.lo;
            int64_t carry = lo < (unsigned long long)a.lo ? 1 : 0;
            a.lo = (int64_t)lo;
            a.hi = a.hi + b.hi + carry;
            break;
        }
    }
    a.cnt += b.cnt;
}

__device__ inline void acc_row(ThreadAcc &a, const AggD &g,
                               const uint8_t *__restrict__ data,
                               const uint8_t *__restrict__ scratch,
                               const uint32_t *__restrict__ rank,
                               const ColLoc *__restrict__ cols, uint32_t row,
                               bool pass)
{
    /* predicated accumulate: operand loads issue unconditionally (so row
     * iterations pipeline with no divergent skip), the fold is masked by
     * `pass` — the row loop in filter_agg_kernel has no continue */
    int64_t iv; double fv;
    switch (g.kind) {
        case CSTRIPE_AGG_COUNT_STAR:
            if (pass) { a.cnt++; a.lo++; }
            break;
        case CSTRIPE_AGG_COUNT_COL: {
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            if (ok & pass) { a.cnt++; a.lo++; }
            break;
        }
        case CSTRIPE_AGG_SUM_I64: {
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            if (ok & pass) {
                acc_add_i128(a, (__int128)iv);
                a.cnt++;
            }
            break;
        }
        case CSTRIPE_AGG_SUM_F64: {
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            if (ok & pass) { a.f += fv; a.cnt++; }
            break;
        }
        case CSTRIPE_AGG_MIN_I64: {
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            if (ok & pass) { a.lo = min(a.lo, iv); a.cnt++; }
            break;
        }
        case CSTRIPE_AGG_MAX_I64: {
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            if (ok & pass) { a.lo = max(a.lo, iv); a.cnt++; }
            break;
        }
        case CSTRIPE_AGG_MIN_F64: {
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            if (ok & pass) {
                if (f64cmp_pg(fv, a.f) < 0) a.f = fv;
                a.cnt++;
            }
            break;
        }
        case CSTRIPE_AGG_MAX_F64: {
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            if (ok & pass) {
                if (f64cmp_pg(fv, a.f) > 0) a.f = fv;
                a.cnt++;
            }
            break;
        }
        case CSTRIPE_AGG_SUM_PROD_I64: {
            int64_t ib; double fb;
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            ok = ok & col_value(data, scratch, rank, cols[g.proj_b], row, ib, fb);
            if (ok & pass) {
                acc_add_i128(a, (__int128)iv * ib);
                a.cnt++;
            }
            break;
        }
        case CSTRIPE_AGG_SUM_DISC_I64: {
            int64_t ib; double fb;
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            ok = ok & col_value(data, scratch, rank, cols[g.proj_b], row, ib, fb);
            if (ok & pass) {
                acc_add_i128(a, (__int128)iv * (g.one - ib));
                a.cnt++;
            }
            break;
        }
        case CSTRIPE_AGG_SUM_DISC_TAX_I64: {
            int64_t ib, ic; double fb, fc;
            bool ok = col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv);
            ok = ok & col_value(data, scratch, rank, cols[g.proj_b], row, ib, fb);
            ok = ok & col_value(data, scratch, rank, cols[g.proj_c], row, ic, fc);
            if (ok & pass) {
                acc_add_i128(a, (__int128)iv * (g.one - ib) * (g.one + ic));
                a.cnt++;
            }
            break;
        }
    }
}

__device__ inline void wave_reduce(ThreadAcc &a, uint8_t kind)
{
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        ThreadAcc b;
        b.lo  = __shfl_down((long long)a.lo, d, WAVE);
        b.hi  = __shfl_down((long long)a.hi, d, WAVE);
        b.f   = __shfl_down(a.f, d, WAVE);
        b.cnt = __shfl_down((long long)a.cnt, d, WAVE);
        acc_merge(a, b, kind);
    }
}

/* the ungrouped kernels' epilogue: wave reduce -> LDS -> wave 0 merges the
 * waves -> one AccCell per aggregate per block, at block_out[block * n_aggs].
 * NL is the LDS row length. UNROLL: the first pass is unrolled over the NA
 * accumulators, guarded by n_aggs where that is no compile-time NA, so they
 * stay in registers; otherwise it is a run-time loop over n_aggs. */
template <int NL, bool UNROLL, int NA>
__device__ __forceinline__ void block_reduce(ThreadAcc (&acc)[NA], const AggParams &params,
                                             uint32_t n_aggs, AccCell *block_out)
{
    __shared__ ThreadAcc lds[AGG_BLOCK / WAVE][NL];
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    #pragma unroll
    for (uint32_t a = 0; a < (UNROLL ? (uint32_t)NA : n_aggs); a++) {
        if (UNROLL && a >= n_aggs) continue;
        wave_reduce(acc[a], params.aggs[a].kind);
        if (lane == 0) lds[wid][a] = acc[a];
    }
    __syncthreads();
    if (wid == 0) {
        for (uint32_t a = lane; a < n_aggs; a += WAVE) {
            ThreadAcc r = lds[0][a];
            for (uint32_t w = 1; w < AGG_BLOCK / WAVE; w++)
                acc_merge(r, lds[w][a], params.aggs[a].kind);
            AccCell c;
            c.lo = r.lo; c.hi = r.hi; c.f = r.f; c.cnt = r.cnt;
            block_out[(uint64_t)blockIdx.x * n_aggs + a] = c;
        }
    }
}

template <int NPREDS, int NAGGS>
__global__ __launch_bounds__(AGG_BLOCK) void filter_agg_kernel(
    const uint8_t *__restrict__ data, const uint8_t *__restrict__ scratch,
    const uint32_t *__restrict__ rank, const GroupDesc *__restrict__ groups,
    const ColLoc *__restrict__ colloc, AccCell *__restrict__ block_out,
    const AggParams params)
{
    /* compile-time trip counts (<0 = runtime) unroll the pred/agg loops so
     * every load is straight-line and pipelines (cdna guide §5.4 trap c) */
    const uint32_t n_preds = NPREDS >= 0 ? (uint32_t)NPREDS : params.n_preds;
    const uint32_t n_aggs = NAGGS >= 0 ? (uint32_t)NAGGS : params.n_aggs;
    const uint32_t gid = blockIdx.x / params.tiles_per_group;
    const uint32_t tile = blockIdx.x % params.tiles_per_group;
    const GroupDesc g = groups[gid];
    const ColLoc *cols = colloc + g.colbase;

    uint32_t row_start = tile * TILE_ROWS;
    uint32_t row_end = min(row_start + TILE_ROWS, g.row_count);

    ThreadAcc acc[NAGGS >= 0 ? NAGGS : MAX_AGGS];
    #pragma unroll
    for (uint32_t a = 0; a < n_aggs; a++) acc_init(acc[a], params.aggs[a].kind);

    for (uint32_t row = row_start + threadIdx.x; row < row_end; row += AGG_BLOCK) {
        bool pass = true, gv = false;
        int last_proj = -1;
        int64_t liv = 0; double lfv = 0; bool lok = false;
        /* no short-circuit: loads stay control-independent so they issue
         * back-to-back and pipeline instead of chaining load->wait->branch.
         * contiguous OR groups accumulate into gv, folded at group end */
        #pragma unroll
        for (uint32_t p = 0; p < n_preds; p++) {
            const PredD &pr = params.preds[p];
            if ((int)pr.proj != last_proj) {   /* BETWEEN reuses the load */
                lok = col_value(data, scratch, rank, cols[pr.proj], row, liv, lfv);
                last_proj = (int)pr.proj;
            }
            gv = gv | (lok && pred_eval(pr, liv, lfv));
            if (pr.gend) { pass = pass & gv; gv = false; }
        }
        if (!pass) continue;
        #pragma unroll
        for (uint32_t a = 0; a < n_aggs; a++)
            acc_row(acc[a], params.aggs[a], data, scratch, rank, cols, row, true);
    }

    block_reduce<MAX_AGGS, (NAGGS >= 0)>(acc, params, n_aggs, block_out);
}


/* =====================================================================
 * FUSED decode -> filter -> partial aggregate: one block
 * decodes a 2048-row tile of ALL projected columns into LDS (one lane per
 * 256 B segment — 64 segments/column/tile, up to 4 i64 columns = 256 lanes)
 * and aggregates straight from LDS. The decompressed stream never touches
 * HBM: eliminates the scratch write + re-read of the two-kernel path.
 * Eligible when every projected column is dense int64 in uniform 256 B LZ4
 * segments (the writer default); otherwise the two-kernel path runs.
 * ===================================================================== */

#define FUSE_TILE_ROWS 2048
#define FUSE_STRIDE 280          /* 8B-aligned per-lane region (val() u64 reads) */

struct FusedTile {
    uint32_t row_count;          /* rows in this tile (<= FUSE_TILE_ROWS) */
    uint32_t seg_base[4];        /* d_segs index of tile's first segment per proj col */
};

template <int NPREDS, int NAGGS>
__global__ __launch_bounds__(AGG_BLOCK) void fused_agg_kernel(
    const uint8_t *__restrict__ data, const SegDesc *__restrict__ segs,
    const FusedTile *__restrict__ tiles, AccCell *__restrict__ block_out,
    int *__restrict__ err, const AggParams params)
{
    const uint32_t n_preds = NPREDS >= 0 ? (uint32_t)NPREDS : params.n_preds;
    const uint32_t n_aggs = NAGGS >= 0 ? (uint32_t)NAGGS : params.n_aggs;
    extern __shared__ uint8_t lds[];                 /* 256 * FUSE_STRIDE */
    const uint32_t tid = threadIdx.x;
    const FusedTile t = tiles[blockIdx.x];

    /* phase 1: decode my segment (lane = col*64 + seg_in_tile) */
    const uint32_t c = tid >> 6;
    const uint32_t sseg = tid & 63;
    const uint32_t nsegs = (t.row_count * 8 + 255) >> 8;
    if (c < params.n_proj && sseg < nsegs) {
        const SegDesc sd = segs[t.seg_base[c] + sseg];
        lz4_lane_decode(data, sd, lds + (size_t)tid * FUSE_STRIDE, err);
    }
    __syncthreads();

    /* phase 2: filter + aggregate from LDS */
    ThreadAcc acc[NAGGS >= 0 ? NAGGS : MAX_AGGS];
    #pragma unroll
    for (uint32_t a = 0; a < n_aggs; a++) acc_init(acc[a], params.aggs[a].kind);

    auto val = [&](uint32_t proj, uint32_t row) -> int64_t {
        const uint32_t region = proj * 64 + (row >> 5);
        return *(const int64_t *)(lds + (size_t)region * FUSE_STRIDE + ((row & 31) << 3));
    };

    for (uint32_t row = tid; row < t.row_count; row += AGG_BLOCK) {
        bool pass = true, gv = false;
        int last_proj = -1;
        int64_t liv = 0;
        for (uint32_t p = 0; p < n_preds; p++) {
            const PredD &pr = params.preds[p];
            if ((int)pr.proj != last_proj) { liv = val(pr.proj, row); last_proj = (int)pr.proj; }
            gv = gv | pred_eval(pr, liv, 0.0);       /* cols are i64: is_float==0 */
            if (pr.gend) { pass = pass & gv; gv = false; }
        }
        if (!pass) continue;
        #pragma unroll
        for (uint32_t a = 0; a < n_aggs; a++) {
            const AggD &g = params.aggs[a];
            ThreadAcc &A = acc[a];
            switch (g.kind) {
                case CSTRIPE_AGG_COUNT_STAR:
                case CSTRIPE_AGG_COUNT_COL:          /* dense: col always present */
                    A.cnt++; A.lo++; break;
                case CSTRIPE_AGG_SUM_I64:
                    acc_add_i128(A, (__int128)val(g.proj_a, row)); A.cnt++; break;
                case CSTRIPE_AGG_MIN_I64:
                    A.lo = min(A.lo, val(g.proj_a, row)); A.cnt++; break;
                case CSTRIPE_AGG_MAX_I64:
                    A.lo = max(A.lo, val(g.proj_a, row)); A.cnt++; break;
                case CSTRIPE_AGG_SUM_PROD_I64:
                    acc_add_i128(A, (__int128)val(g.proj_a, row) * val(g.proj_b, row));
                    A.cnt++; break;
                case CSTRIPE_AGG_SUM_DISC_I64:
                    acc_add_i128(A, (__int128)val(g.proj_a, row) * (g.one - val(g.proj_b, row)));
                    A.cnt++; break;
                case CSTRIPE_AGG_SUM_DISC_TAX_I64:
                    acc_add_i128(A, (__int128)val(g.proj_a, row) * (g.one - val(g.proj_b, row))
                                     * (g.one + val(g.proj_c, row)));
                    A.cnt++; break;
                default: break;                       /* host guards float kinds */
            }
        }
    }

    block_reduce<MAX_AGGS, (NAGGS >= 0)>(acc, params, n_aggs, block_out);
}

/* ---- R-row variant (R=8): one (R-1)*step+8 <= 57 B window per column.
 * step in {4..7} is wave-uniform per column, so a 4-way uniform branch gives
 * each extraction COMPILE-TIME shift amounts (no dynamic register indexing,
 * no scratch). Doubles in-flight loads again over the quad kernel. ---- */

/* raw per-row values: int columns store the integer, float columns store
 * the double's BIT PATTERN (converted only at use) — halves the register
 * footprint of a staged row group, which is what caps occupancy here */
template <int R>
struct ValsR {
    int64_t v[R];
    __device__ inline double fget(int k) const {
        double d;
        __builtin_memcpy(&d, &v[k], 8);
        return d;
    }
};

template <int R, uint32_t STEP>
__device__ inline void canon_extract(const uint8_t *__restrict__ sp,
                                     uint32_t pos, uint64_t m, uint64_t hval,
                                     uint64_t (&r)[R])
{
    /* per-u64 window loads (measured faster than 16 B dwordx4 quads here:
     * the unaligned quads span more lines per instruction and raised the
     * kernel's spill pressure for no latency win) */
    constexpr uint32_t NW = ((R - 1) * STEP + 8 + 7) / 8;
    uint64_t w[NW];
    #pragma unroll
    for (uint32_t i = 0; i < NW; i++)
        __builtin_memcpy(&w[i], sp + pos + 8 * i, 8);
    #pragma unroll
    for (uint32_t k = 0; k < R; k++) {
        const uint32_t d = k * STEP;
        const uint32_t wi = d >> 3, sh = (d & 7u) * 8u;
        uint64_t raw = sh ? ((w[wi] >> sh) | (w[wi + 1 < NW ? wi + 1 : wi] << (64u - sh)))
                          : w[wi];
        r[k] = (raw & m) | hval;
    }
}

template <int R>
__device__ inline void col_multi(const uint8_t *__restrict__ data,
                                 const uint8_t *__restrict__ scratch,
                                 const ColLoc &cl, uint32_t row, ValsR<R> &q)
{
    const uint8_t *base = (cl.flags & 1) ? scratch + cl.val_off : data + cl.val_off;
    if ((cl.flags & 4) && cl.mode != CSF_SEGMODE_LIT) {
        if ((cl.mode & 0xF8u) == CSF_SEGMODE_ZR4B_BASE) {
            /* width-4 single-varying-byte / const slots (char(1) flags):
             * ONE u64 window load covers 8 rows' varying bytes (stride 1) */
            const uint32_t kk = cl.L;
            uint32_t slots[R];
            if (cl.mode == CSF_SEGMODE_ZR4_CONST) {
                #pragma unroll
                for (int k = 0; k < R; k++) slots[k] = (uint32_t)cl.hval;
            } else if (row == 0) {
                #pragma unroll
                for (int k = 0; k < R; k++) {
                    const uint32_t j = row + (uint32_t)k;
                    const uint32_t pos = 15u + (j == 0 ? kk : j + 3u + kk);
                    slots[k] = (uint32_t)cl.hval |
                               ((uint32_t)base[pos] << (8u * kk));
                }
            } else {
                uint64_t w[(R + 7) / 8];
                #pragma unroll
                for (int i = 0; i < (R + 7) / 8; i++)
                    __builtin_memcpy(&w[i], base + 15u + row + 3u + kk + 8u * i, 8);
                #pragma unroll
                for (int k = 0; k < R; k++)
                    slots[k] = (uint32_t)cl.hval |
                               ((uint32_t)((w[k >> 3] >> (8 * (k & 7))) & 0xFFu)
                                << (8u * kk));
            }
            #pragma unroll
            for (int k = 0; k < R; k++) {
                if (cl.type == CSTRIPE_F32) {
                    float ff;
                    __builtin_memcpy(&ff, &slots[k], 4);
                    const double d = ff;
                    __builtin_memcpy(&q.v[k], &d, 8);
                } else if (cl.type == CSTRIPE_TEXT) {
                    q.v[k] = (int64_t)slots[k];
                } else {
                    q.v[k] = (int64_t)(int32_t)slots[k];
                }
            }
            return;
        }
        uint64_t r[R];
        if (cl.mode == CSF_SEGMODE_CONST || cl.mode == CSF_SEGMODE_ZR_CONST) {
            #pragma unroll
            for (int k = 0; k < R; k++) r[k] = (uint64_t)cl.hval;
        } else if ((cl.mode & 0xF0u) == CSF_SEGMODE_ZRP_BASE) {
            /* zstd P(L): dense low-L bytes in the literal section, byte
             * stride L (canon_pos); only j=0 is special */
            const uint32_t Lx = cl.L;
            const uint64_t m = (~0ull) >> ((8u - Lx) * 8u);
            if (row == 0) {
                #pragma unroll
                for (int k = 0; k < R; k++) {
                    uint64_t a;
                    __builtin_memcpy(&a, base + canon_pos(cl.mode, Lx, row + k), 8);
                    r[k] = (a & m) | (uint64_t)cl.hval;
                }
            } else {
                const uint32_t pos = 23u + (row - 1u) * Lx;
                switch (Lx) {                 /* wave-uniform */
                    case 1: canon_extract<R, 1>(base, pos, m, (uint64_t)cl.hval, r); break;
                    case 2: canon_extract<R, 2>(base, pos, m, (uint64_t)cl.hval, r); break;
                    case 3: canon_extract<R, 3>(base, pos, m, (uint64_t)cl.hval, r); break;
                    default: canon_extract<R, 4>(base, pos, m, (uint64_t)cl.hval, r); break;
                }
            }
        } else {                              /* lz4 P(L) */
            const uint32_t Lx = cl.L, step = Lx + 3u;
            const uint64_t m = (~0ull) >> ((8u - Lx) * 8u);
            if (row < 2) {                    /* j=0 -> 1, j=1 -> 9 specials */
                #pragma unroll
                for (int k = 0; k < R; k++) {
                    const uint32_t j = row + k;
                    uint32_t pos = j * step + (6u - Lx);
                    pos = j == 0 ? 1u : (j == 1 ? 9u : pos);
                    uint64_t a;
                    __builtin_memcpy(&a, base + pos, 8);
                    r[k] = (a & m) | (uint64_t)cl.hval;
                }
            } else {
                const uint32_t pos = row * step + (6u - Lx);
                /* wave-uniform branch on step -> compile-time shifts */
                switch (step) {
                    case 4: canon_extract<R, 4>(base, pos, m, (uint64_t)cl.hval, r); break;
                    case 5: canon_extract<R, 5>(base, pos, m, (uint64_t)cl.hval, r); break;
                    case 6: canon_extract<R, 6>(base, pos, m, (uint64_t)cl.hval, r); break;
                    default: canon_extract<R, 7>(base, pos, m, (uint64_t)cl.hval, r); break;
                }
            }
        }
        #pragma unroll
        for (int k = 0; k < R; k++) q.v[k] = (int64_t)r[k];   /* F64: bits */
        return;
    }
    if (cl.flags & 4) base += (uint64_t)cl.hval;     /* LIT header */
    switch (cl.type) {                                /* row % R == 0 */
        case CSTRIPE_I8: {
            const int8_t *p = (const int8_t *)base + row;
            #pragma unroll
            for (int k = 0; k < R; k++) q.v[k] = p[k];
            break;
        }
        case CSTRIPE_I16: {
            const int16_t *p = (const int16_t *)base + row;
            #pragma unroll
            for (int k = 0; k < R; k++) q.v[k] = p[k];
            break;
        }
        case CSTRIPE_I32: {
            const int32_t *p = (const int32_t *)base + row;
            #pragma unroll
            for (int k = 0; k < R; k++) q.v[k] = p[k];
            break;
        }
        case CSTRIPE_I64: {
            const uint8_t *p = base + (size_t)row * 8;
            #pragma unroll
            for (int k = 0; k < R; k += 2) {
                struct { int64_t a, b; } t;
                __builtin_memcpy(&t, p + 16 * (k / 2), 16);
                q.v[k] = t.a;
                if (k + 1 < R) q.v[k + 1] = t.b;
            }
            break;
        }
        case CSTRIPE_F32: {
            const float *p = (const float *)base + row;
            #pragma unroll
            for (int k = 0; k < R; k++) {
                const double d = p[k];
                __builtin_memcpy(&q.v[k], &d, 8);     /* widen, store bits */
            }
            break;
        }
        case CSTRIPE_TEXT: {
            const uint32_t *p = (const uint32_t *)base + row;
            #pragma unroll
            for (int k = 0; k < R; k++) q.v[k] = (int64_t)p[k];
            break;
        }
        default: {                                    /* F64 bits */
            const uint8_t *p = base + (size_t)row * 8;
            #pragma unroll
            for (int k = 0; k < R; k += 2) {
                struct { int64_t a, b; } t;
                __builtin_memcpy(&t, p + 16 * (k / 2), 16);
                q.v[k] = t.a;
                if (k + 1 < R) q.v[k + 1] = t.b;
            }
            break;
        }
    }
}

template <int R>
__device__ inline void acc_multi(ThreadAcc &a, const AggD &g,
                                 const uint8_t *__restrict__ data,
                                 const uint8_t *__restrict__ scratch,
                                 const ColLoc *__restrict__ cols, uint32_t row,
                                 const bool (&pv)[R])
{
    ValsR<R> qa, qb, qc;
    int64_t c = 0;
    #pragma unroll
    for (int k = 0; k < R; k++) c += (int)pv[k];
    switch (g.kind) {
        case CSTRIPE_AGG_COUNT_STAR:
        case CSTRIPE_AGG_COUNT_COL:
            a.cnt += c;
            a.lo += c;
            return;
        case CSTRIPE_AGG_SUM_I64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k]) acc_add_i128(a, (__int128)qa.v[k]);
            break;
        case CSTRIPE_AGG_SUM_F64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k]) a.f += qa.fget(k);
            break;
        case CSTRIPE_AGG_MIN_I64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k]) a.lo = min(a.lo, qa.v[k]);
            break;
        case CSTRIPE_AGG_MAX_I64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k]) a.lo = max(a.lo, qa.v[k]);
            break;
        case CSTRIPE_AGG_MIN_F64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k] && f64cmp_pg(qa.fget(k), a.f) < 0) a.f = qa.fget(k);
            break;
        case CSTRIPE_AGG_MAX_F64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k] && f64cmp_pg(qa.fget(k), a.f) > 0) a.f = qa.fget(k);
            break;
        case CSTRIPE_AGG_SUM_PROD_I64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            col_multi<R>(data, scratch, cols[g.proj_b], row, qb);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k]) acc_add_i128(a, (__int128)qa.v[k] * qb.v[k]);
            break;
        case CSTRIPE_AGG_SUM_DISC_I64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            col_multi<R>(data, scratch, cols[g.proj_b], row, qb);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k]) acc_add_i128(a, (__int128)qa.v[k] * (g.one - qb.v[k]));
            break;
        case CSTRIPE_AGG_SUM_DISC_TAX_I64:
            col_multi<R>(data, scratch, cols[g.proj_a], row, qa);
            col_multi<R>(data, scratch, cols[g.proj_b], row, qb);
            col_multi<R>(data, scratch, cols[g.proj_c], row, qc);
            #pragma unroll
            for (int k = 0; k < R; k++)
                if (pv[k]) acc_add_i128(a, (__int128)qa.v[k] * (g.one - qb.v[k])
                                           * (g.one + qc.v[k]));
            break;
        default:
            break;
    }
    a.cnt += c;
}

template <int NPREDS, int NAGGS, int R, int MINW = 1>
__global__ __launch_bounds__(AGG_BLOCK, MINW) void multi_agg_kernel(
    const uint8_t *__restrict__ data, const uint8_t *__restrict__ scratch,
    const GroupDesc *__restrict__ groups, const ColLoc *__restrict__ colloc,
    AccCell *__restrict__ block_out, const AggParams params)
{
    const uint32_t n_preds = NPREDS >= 0 ? (uint32_t)NPREDS : params.n_preds;
    const uint32_t n_aggs = NAGGS >= 0 ? (uint32_t)NAGGS : params.n_aggs;
    const uint32_t gid = blockIdx.x / params.tiles_per_group;
    const uint32_t tile = blockIdx.x % params.tiles_per_group;
    const GroupDesc g = groups[gid];
    const ColLoc *cols = colloc + g.colbase;

    const uint32_t row_start = tile * TILE_ROWS;
    const uint32_t row_end = min(row_start + TILE_ROWS, g.row_count);

    ThreadAcc acc[NAGGS >= 0 ? NAGGS : MAX_AGGS];
    #pragma unroll
    for (uint32_t a = 0; a < n_aggs; a++) acc_init(acc[a], params.aggs[a].kind);

    for (uint32_t row = row_start + R * threadIdx.x; row < row_end;
         row += R * AGG_BLOCK) {
        bool pv[R], gv[R];
        #pragma unroll
        for (int k = 0; k < R; k++) { pv[k] = row + k < row_end; gv[k] = false; }
        int last_proj = -1;
        ValsR<R> q{};
        #pragma unroll
        for (uint32_t p = 0; p < n_preds; p++) {
            const PredD &pr = params.preds[p];
            if ((int)pr.proj != last_proj) {
                col_multi<R>(data, scratch, cols[pr.proj], row, q);
                last_proj = (int)pr.proj;
            }
            #pragma unroll
            for (int k = 0; k < R; k++)
                gv[k] = gv[k] | pred_eval(pr, q.v[k], q.fget(k));
            if (pr.gend) {
                #pragma unroll
                for (int k = 0; k < R; k++) { pv[k] = pv[k] & gv[k]; gv[k] = false; }
                /* early wave exit: if every lane's window is dead after
                 * this AND-group, skip the remaining pred columns' loads
                 * and evals (wave-uniform ballot branch) */
                bool alive = false;
                #pragma unroll
                for (int k = 0; k < R; k++) alive |= pv[k];
                if (__ballot(alive) == 0) break;
            }
        }
        bool any = false;
        #pragma unroll
        for (int k = 0; k < R; k++) any |= pv[k];
        if (__ballot(any) == 0) continue;
        #pragma unroll
        for (uint32_t a = 0; a < n_aggs; a++)
            acc_multi<R>(acc[a], params.aggs[a], data, scratch, cols, row, pv);
    }

    block_reduce<MAX_AGGS, (NAGGS >= 0)>(acc, params, n_aggs, block_out);
}

/* =====================================================================
 * Dense overlapped body (multi_agg_kernel_ov) — for scans whose every
 * referenced column is, in every selected chunk group, a dense I64 canonical
 * P(L) / CONST stream (lz4 or zstd). The host resolves the query into SLOTS
 * (distinct projected columns, predicate slots first), so a column is loaded
 * once per row group however many predicates and operands name it.
 *
 * A work item is one (chunk group, R*AGG_BLOCK-row tile), 2048 rows at R=8.
 * Lane t holds rows t, t+256, ..., t+(R-1)*256 of the tile, so consecutive
 * lanes hold consecutive rows and a wave's load covers 64*step contiguous
 * bytes. A fixed grid walks items blockIdx.x, +gridDim.x, ... with a plain
 * for; every trip count follows from n_items. Per item:
 *   1. the predicate-slot dwords (issued one item earlier) are masked down,
 *   2. the NEXT item's predicate-slot dwords are issued back to back,
 *   3. descriptors are fetched ahead (ColLoc two items, GroupDesc three),
 *   4. all predicates are evaluated from registers, each as one unsigned
 *      32-bit range test of the row's low word (ov_cmp); if any lane of the
 *      wave passes, the lanes that hold a passing row load those rows of the
 *      operand-only slots and fold them.
 * The wait in (4) therefore covers this item's operands and the next item's
 * predicate dwords together: one exposed round trip per item.
 *
 * A P(L) value is hval | low-L-bytes with L <= 4, so a row is one u32 per
 * slot: the unaligned dword at its closed-form position, masked (ov_load).
 * ===================================================================== */

#define OV_R        8                    /* rows per lane per work item */
#define OV_R_ANY    4                    /* ... of the unspecialised instance:
                                          * half the registers per row group */
#define OV_MAX_SLOTS 4
#define OV_MAX_AGGS 4

struct OvPlan {
    uint32_t n_items;                    /* n_groups * tiles_pg */
    uint32_t tiles_pg;                   /* ceil(largest group / (R * AGG_BLOCK)) */
    uint32_t n_slots, n_pslots;          /* slots [0, n_pslots) carry predicates */
    uint8_t slot_proj[OV_MAX_SLOTS];
    /* predicates as whole aligned words, so that a run-time predicate index
     * is a plain scalar word load: slot | op << 8 | gend << 16, and ival */
    uint32_t pred_ctl[MAX_PREDS];
    int64_t pred_val[MAX_PREDS];
    uint8_t agg_slot[OV_MAX_AGGS][4];    /* slots of proj_a, proj_b, proj_c */
    uint32_t ksig;                       /* the shape words (ov_sig_*), host */
    uint64_t sig;                        /* side: pick a specialised instance */
};

/* one slot of one chunk group, wave-uniform, four SGPRs:
 * meta = stream offset in d_data (48 bits) | step << 48 | zstd << 56, where
 * step = bytes between consecutive rows' low bytes (0 = CONST) */
struct OvCol {
    uint64_t meta;
    uint64_t hval;
};

/* the ColLoc fields ov_col needs, as fetched: the fetch and the packing are
 * kept a loop trip apart so that no wait sits right behind the scalar loads */
struct OvRaw {
    uint64_t val_off;
    uint64_t hval;
    uint32_t ml;        /* mode | L << 8 */
};

__device__ inline OvRaw ov_fetch(const ColLoc &cl)
{
    /* mode and L as one aligned word: byte-sized fields would each be a
     * vector load with a full wait behind it, under the windows in flight */
    static_assert(offsetof(ColLoc, mode) % 4 == 0 &&
                  offsetof(ColLoc, L) == offsetof(ColLoc, mode) + 1, "ColLoc layout");
    OvRaw r;
    r.val_off = cl.val_off;
    r.hval = (uint64_t)cl.hval;
    __builtin_memcpy(&r.ml, &cl.mode, 4);
    return r;
}

__device__ inline OvCol ov_col(const OvRaw &r)
{
    const uint32_t mode = r.ml & 0xFFu, L = (r.ml >> 8) & 0xFFu;
    const uint32_t zr = mode >= CSF_SEGMODE_ZRP_BASE ? 1u : 0u;
    const bool cst = mode == CSF_SEGMODE_CONST || mode == CSF_SEGMODE_ZR_CONST;
    const uint32_t step = cst ? 0u : (zr ? L : L + 3u);
    OvCol c;
    c.meta = r.val_off | ((uint64_t)step << 48) | ((uint64_t)zr << 56);
    c.hval = r.hval;
    return c;
}

__device__ inline uint32_t ov_step(const OvCol &c) { return (uint32_t)(c.meta >> 48) & 0xFFu; }
__device__ inline uint32_t ov_zr(const OvCol &c) { return (uint32_t)(c.meta >> 56); }
__device__ inline uint64_t ov_off(const OvCol &c) { return c.meta & 0xFFFFFFFFFFFFull; }
/* low bytes of row j >= 2 (zstd: j >= 1) start at j*step + ov_off0 (canon_pos) */
__device__ inline uint32_t ov_off0(uint32_t step, uint32_t zr) { return (zr ? 23u : 9u) - step; }
/* low-L-bytes mask; 0 for a CONST slot (the value is hval alone) */
__device__ inline uint32_t ov_mask(uint32_t step, uint32_t zr)
{
    const uint32_t L = zr ? step : step - 3u;
    return step == 0 ? 0u : 0xFFFFFFFFu >> ((4u - L) * 8u);
}

/* One slot's dwords for a tile: lane t takes rows row0 + k*AGG_BLOCK + t,
 * k < R, so one load instruction of a wave covers 64*step contiguous bytes and
 * the R loads walk the stream front to back, every line fetched once. A P(L)
 * value has L <= 4 variable bytes, so the unaligned dword at the row's
 * closed-form position (canon_pos) is the whole row: no neighbour word, no
 * shift. The address is one wave-uniform base (stream + row0*step) plus a
 * 32-bit lane offset that advances by AGG_BLOCK*step per k. Only row 0 of a
 * stream sits off the closed form (lz4: +1, zstd: +15; lz4 row 1 is at
 * 9 = off0 + step): a per-lane offset select for k == 0 of the group's first
 * tile.
 * rows: bit k set = load row k. The predicate slots pass the rows inside the
 * group (all of them except in a group's last tile), the operand-only slots
 * the rows that passed. There is one code path for both and for full and
 * last tiles alike: two paths that load the same registers meet in a merge,
 * a merge costs a copy, and a copy of a loaded register a wait right behind
 * the load.
 * Reach: a row whose bit is clear loads nothing, and a loaded row reads the
 * 4 bytes at the position where the windowed bodies read 8, so this never
 * reads a byte of a stream that they do not. */
template <int R>
__device__ inline void ov_load(const uint8_t *__restrict__ data, const OvCol &c,
                               uint32_t row0, uint32_t rows, uint32_t (&w)[R])
{
    const uint32_t step = ov_step(c), zr = ov_zr(c);
    if (step == 0) return;                    /* CONST: no load, lo = 0 */
    const uint8_t *sb = data + (ov_off(c) + (uint64_t)(row0 * step));
    uint32_t vo = ov_off0(step, zr) + threadIdx.x * step;
    const uint32_t vo0 = (row0 == 0 && threadIdx.x == 0) ? (zr ? 15u : 1u) : vo;
    #pragma unroll
    for (uint32_t k = 0; k < (uint32_t)R; k++) {
        if ((rows >> k) & 1u)
            __builtin_memcpy(&w[k], sb + (k == 0 ? vo0 : vo), 4);
        vo += AGG_BLOCK * step;
    }
}

/* bit k = row row0 + k*AGG_BLOCK + t lies inside the group (row0 < rc) */
template <int R>
__device__ inline uint32_t ov_rows(uint32_t row0, uint32_t rc)
{
    const uint32_t left = rc - row0;
    uint32_t m = 0;
    #pragma unroll
    for (uint32_t k = 0; k < (uint32_t)R; k++)
        m |= (uint32_t)(k * AGG_BLOCK + threadIdx.x < left) << k;
    return m;
}

/* dwords -> the rows' low words (value = hval | low word); CONST: all zero.
 * The empty asm pins each AND here: left alone, the compiler sinks it to its
 * first use, past the next item's loads, which then need a second register
 * set and a copy per dword to keep w alive. */
template <int R>
__device__ inline void ov_lows(const OvCol &c, const uint32_t (&w)[R], uint32_t (&lo)[R])
{
    const uint32_t m = ov_mask(ov_step(c), ov_zr(c));
    #pragma unroll
    for (int k = 0; k < R; k++) {
        lo[k] = w[k] & m;
        asm volatile("" : "+v"(lo[k]));
    }
}

/* slot -> registers: wave-uniform compare chain over compile-time slots */
template <int R, int NS>
__device__ inline void ov_pick(const uint32_t (&lo)[NS][R], const OvCol (&c)[NS],
                               uint32_t slot, uint32_t (&o)[R], uint64_t &h)
{
    #pragma unroll
    for (int s = 0; s < NS; s++)
        if (slot == (uint32_t)s) {
            #pragma unroll
            for (int k = 0; k < R; k++) o[k] = lo[s][k];
            h = c[s].hval;
        }
}

__device__ inline int64_t ov_val(uint32_t lo, uint64_t h) { return (int64_t)((uint64_t)lo | h); }

/* the low-word mask of a slot: the largest low word any of its rows holds */
template <int NS>
__device__ inline uint32_t ov_pick_mask(const OvCol (&c)[NS], uint32_t slot)
{
    uint32_t m = 0;
    #pragma unroll
    for (int s = 0; s < NS; s++)
        if (slot == (uint32_t)s) m = ov_mask(ov_step(c[s]), ov_zr(c[s]));
    return m;
}

/* SUM_PROD of a specialised instance takes a narrow fold when, for the whole
 * row group, both operands are their low words alone (hval == 0, so neither
 * is negative) and their widths add to at most 61 bits: a product is then
 * below 2^61 and eight of them below 2^64, so the row group folds in one u64
 * with 32-bit multiply-adds (a failing row adds 0) and meets the 128-bit
 * accumulator once. Wave-uniform; anything else takes the 128-bit fold, and
 * so does the unspecialised instance, which the second fold made slower
 * (registers spilled: DESIGN section 3). */
#define OV_NARROW_BITS 61u

/* row k's low word if the row passed, else 0 */
__device__ inline uint32_t ov_sel(uint32_t pv, int k, uint32_t x)
{
    return ((pv >> k) & 1u) ? x : 0u;
}

/* one predicate against one slot of one chunk group, reduced on the scalar
 * side (op, hval and ival are all wave-uniform) to an unsigned range test of
 * the row's low word: the row passes iff ((lo - a) <= d) != inv.
 * A value is hval | lo with lo a u32, so its high word is hval's: where that
 * differs from ival's (as signed words) the predicate is constant for the row
 * group; where it is equal the low words x = lo | (u32)hval decide, unsigned,
 * and the predicate holds on a range [A, B] of x or on its complement.
 * hval has the slot's low L bytes clear (and a CONST slot's lo is 0), so
 * x = lo + (u32)hval and the bias folds into a. Exact for every int64 ival. */
struct OvCmp {
    uint32_t a, d, inv;
};

__device__ inline OvCmp ov_cmp(uint32_t op, uint64_t hval, int64_t ival)
{
    const int32_t vh = (int32_t)(hval >> 32), ih = (int32_t)((uint64_t)ival >> 32);
    const uint32_t t = (uint32_t)ival;
    uint32_t A = 0, B = 0xFFFFFFFFu;
    bool none = false, inv = false;
    if (vh != ih) {
        const bool less = vh < ih;            /* every row < ival, or every row > */
        switch (op) {
            case CSTRIPE_PRED_LT: case CSTRIPE_PRED_LE: none = !less; break;
            case CSTRIPE_PRED_GT: case CSTRIPE_PRED_GE: none = less; break;
            case CSTRIPE_PRED_EQ: none = true; break;
            default: break;
        }
    } else {
        switch (op) {
            case CSTRIPE_PRED_LT: none = t == 0; B = t - 1u; break;
            case CSTRIPE_PRED_LE: B = t; break;
            case CSTRIPE_PRED_GT: none = t == 0xFFFFFFFFu; A = t + 1u; break;
            case CSTRIPE_PRED_GE: A = t; break;
            case CSTRIPE_PRED_EQ: A = B = t; break;
            default: A = B = t; inv = true; break;
        }
    }
    if (none) { A = 0; B = 0xFFFFFFFFu; inv = true; }
    OvCmp r;
    r.a = A - (uint32_t)hval;
    r.d = B - A;
    r.inv = inv ? 1u : 0u;
    return r;
}

/* integer kinds only: ThreadAcc.f stays the constant acc_init gives them */
__device__ inline void ov_acc_init(ThreadAcc &a, uint8_t kind)
{
    a.lo = kind == CSTRIPE_AGG_MIN_I64 ? INT64_MAX
         : kind == CSTRIPE_AGG_MAX_I64 ? INT64_MIN : 0;
    a.hi = 0; a.f = 0.0; a.cnt = 0;
}

/* a query's shape as compile-time words, for the specialised instances:
 * SIG  = slot of predicate p at bits [2p, 2p+2), slot of aggregate a's
 *        operand k at bits [32+6a+2k, +2);  KSIG = kind of aggregate a at
 *        bits [4a, 4a+4) */
__host__ __device__ constexpr uint64_t ov_sig_pred(uint32_t p, uint32_t slot)
{
    return (uint64_t)slot << (2u * p);
}
__host__ __device__ constexpr uint64_t ov_sig_op(uint32_t a, uint32_t k, uint32_t slot)
{
    return (uint64_t)slot << (32u + 6u * a + 2u * k);
}
__host__ __device__ constexpr uint32_t ov_ksig(uint32_t a, uint32_t kind)
{
    return kind << (4u * a);
}

/* ---------------------------------------------------------------------
 * The window form of the loads, kept for scans over zstd canonical streams.
 * There a row's low bytes are step = L = 1..4 bytes apart (lz4: L+3), so a
 * per-lane 8-row window is one to four u64 words where the lane-contiguous
 * form above issues eight dword loads per slot: on Q6 over 1B zstd rows the
 * lane-contiguous form measured 2.84 ms against 2.74 ms for this one
 * (DESIGN section 3). Lane t holds rows R*t .. R*t+R-1 of the tile.
 * --------------------------------------------------------------------- */

/* u64 words of the widest (step 7) window of an R-row group */
#define OV_NW(R)    ((((R) - 1) * 7 + 4 + 7) / 8)

template <int R, uint32_t STEP>
__device__ inline void ov_extract(const uint64_t (&w)[OV_NW(R)], uint32_t m,
                                  uint32_t (&lo)[R])
{
    #pragma unroll
    for (uint32_t k = 0; k < (uint32_t)R; k++) {
        const uint32_t d = k * STEP, wi = d >> 3, sh = (d & 7u) * 8u;
        uint32_t x = (uint32_t)(w[wi] >> sh);
        if (sh > 32u) x |= (uint32_t)(w[wi + 1 < OV_NW(R) ? wi + 1 : wi] << (64u - sh));
        lo[k] = x & m;
    }
}

/* issue one slot's window for the lane's row group (row % R == 0, row inside
 * the chunk group). Every word is loaded straight into its final register
 * under a wave-uniform guard, never merged across branches: a merge would
 * cost a copy, and a copy of a loaded register a wait right behind the load.
 * Rows 0/1 of an lz4 stream and row 0 of a zstd one sit at their own offsets
 * (canon_pos). The one lane that holds row 0 points word 0 — which only
 * rows 0/1 of an lz4 window touch, step being >= 4 there — at lz4 row 0, and
 * loads lz4 row 1 / zstd row 0 into fx.
 * Word 0 is issued LAST and ov_take reads it on every path, so that one
 * read stands for "the whole window has landed" (loads return in order):
 * nothing of a window then counts as outstanding when the next one is
 * issued into the same registers, and no wait lands between the loads.
 * ALL (the operand-only slots, whose window is consumed at once): no guards
 * either — a surplus word re-reads the window's last word, so the reach is
 * the same and the extraction cannot be sunk in between the loads. */
template <int R, bool ALL>
__device__ inline void ov_issue(const uint8_t *__restrict__ data, const OvCol &c,
                                uint32_t row, uint64_t (&w)[OV_NW(R)], uint32_t &fx)
{
    const uint32_t step = ov_step(c), zr = ov_zr(c);
    if (step == 0) return;
    const uint8_t *base = data + ov_off(c);
    const uint8_t *p = base + (row * step + ov_off0(step, zr));
    const uint32_t nbytes = (R - 1) * step + 4u;
    if (row == 0) __builtin_memcpy(&fx, base + (zr ? 15u : 9u), 4);
    const uint32_t lastw = (nbytes - 1u) >> 3;
    #pragma unroll
    for (uint32_t i = OV_NW(R) - 1; i >= 1; i--) {
        if (ALL) __builtin_memcpy(&w[i], p + 8u * min(i, lastw), 8);
        else if (8u * i < nbytes) __builtin_memcpy(&w[i], p + 8u * i, 8);
    }
    __builtin_memcpy(&w[0], (row == 0 && !zr) ? base + 1 : p, 8);
    /* keep the scheduler from pulling a first use up between the loads */
    __builtin_amdgcn_sched_barrier(0);
}

/* window -> the row group's R low words (value = hval | low word) */
template <int R>
__device__ inline void ov_take(const OvCol &c, uint32_t row,
                               const uint64_t (&w)[OV_NW(R)], uint32_t fx,
                               uint32_t (&lo)[R])
{
    const uint32_t step = ov_step(c), zr = ov_zr(c);
    const uint32_t m = ov_mask(step, zr);     /* CONST: any arm, all zero */
    switch (step) {                           /* wave-uniform */
        case 1: ov_extract<R, 1>(w, m, lo); break;
        case 2: ov_extract<R, 2>(w, m, lo); break;
        case 3: ov_extract<R, 3>(w, m, lo); break;
        case 4: ov_extract<R, 4>(w, m, lo); break;
        case 5: ov_extract<R, 5>(w, m, lo); break;
        case 6: ov_extract<R, 6>(w, m, lo); break;
        default: ov_extract<R, 7>(w, m, lo); break;
    }
    if (row == 0) {
        if (zr) lo[0] = fx & m;
        else    lo[1] = fx & m;
    }
}

/* WIN: the window form of the loads (ov_issue / ov_take), else the
 * lane-contiguous form (ov_rows / ov_load / ov_lows). Only the loads, the
 * initial row mask and the rotate of the loaded words differ, each under an
 * if constexpr below; the plan, the descriptor pipeline, the predicates, the
 * folds and the reduce exist once.
 * EXACT: the template counts, SIG and KSIG are the query's, so every slot
 * and kind below is a compile-time constant; otherwise the counts are
 * capacities and everything comes from the plan / params through
 * wave-uniform guards */
template <bool WIN, int R, int NS, int NPS, int NPREDS, int NAGGS, bool EXACT, int MINW,
          uint64_t SIG = 0, uint32_t KSIG = 0>
__global__ __launch_bounds__(AGG_BLOCK, MINW) void multi_agg_kernel_ov(
    const uint8_t *__restrict__ data, const GroupDesc *__restrict__ groups,
    const ColLoc *__restrict__ colloc, AccCell *__restrict__ block_out,
    const AggParams params, const OvPlan plan)
{
    constexpr uint32_t TILE = R * AGG_BLOCK;
    const uint32_t ns = EXACT ? (uint32_t)NS : plan.n_slots;
    const uint32_t nps = EXACT ? (uint32_t)NPS : plan.n_pslots;
    const uint32_t n_preds = EXACT ? (uint32_t)NPREDS : params.n_preds;
    const uint32_t n_aggs = EXACT ? (uint32_t)NAGGS : params.n_aggs;
    const uint32_t n_items = plan.n_items, tpg = plan.tiles_pg;
    const uint32_t G = gridDim.x, last = n_items - 1u;
    /* the lane's first row within a tile: the window form gives lane t rows
     * R*t .. R*t+R-1, the lane form rows t + k*AGG_BLOCK off a uniform base */
    const uint32_t lrow = WIN ? R * threadIdx.x : 0u;

    ThreadAcc acc[NAGGS];
    #pragma unroll
    for (int a = 0; a < NAGGS; a++) ov_acc_init(acc[a], params.aggs[a].kind);

    /* prologue: the block's first item, and the descriptors behind it */
    uint32_t it = blockIdx.x;
    OvCol c[NS] = {};
    /* crow: the lane's first row (window form), the tile's first row, uniform
     * (lane form) */
    uint32_t crc = 0, crow = 0;
    /* both forms' load state is declared here so that it reaches the rotate;
     * the form not instantiated never uses its half, which dies.
     * Lane form: crows, bit k = row crow + k*AGG_BLOCK + t exists, and the
     * dwords wn, zeroed word by word: an aggregate initialiser makes the whole
     * array one 32-dword vector value, copied wholesale behind a full wait
     * every trip.
     * Window form: the windows ww and the off-form rows fx (ov_issue). */
    uint32_t crows = 0;
    uint32_t wn[NS][R];
    #pragma unroll
    for (int s = 0; s < NS; s++) {
        #pragma unroll
        for (int k = 0; k < R; k++) wn[s][k] = 0;
    }
    uint64_t ww[NS][OV_NW(R)] = {};
    uint32_t fx[NS] = {};
    if (it < n_items) {
        const GroupDesc g0 = groups[it / tpg];
        crc = g0.row_count;
        crow = (it % tpg) * TILE + lrow;
        #pragma unroll
        for (int s = 0; s < NS; s++)
            if ((uint32_t)s < ns) c[s] = ov_col(ov_fetch(colloc[g0.colbase + plan.slot_proj[s]]));
        if constexpr (WIN) {
            if (crow < crc) {
                #pragma unroll
                for (int s = 0; s < NS; s++)
                    if ((uint32_t)s < nps) ov_issue<R, false>(data, c[s], crow, ww[s], fx[s]);
            }
        } else {
            if (crow < crc) crows = ov_rows<R>(crow, crc);
            #pragma unroll
            for (int s = 0; s < NS; s++)
                if ((uint32_t)s < nps) ov_load<R>(data, c[s], crow, crows, wn[s]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    /* indices past the end are clamped for the descriptor reads only; an
     * item that does not exist has an empty row mask (lane form) or no
     * window issued (window form) and loads nothing */
    const GroupDesc g1 = groups[min(it + G, last) / tpg];
    OvCol nc[NS] = {};
    #pragma unroll
    for (int s = 0; s < NS; s++)
        if ((uint32_t)s < ns) nc[s] = ov_col(ov_fetch(colloc[g1.colbase + plan.slot_proj[s]]));
    uint32_t nrc = g1.row_count;
    GroupDesc g2 = groups[min(it + 2u * G, last) / tpg];

    for (; it < n_items; it += G) {
        /* 1. this item's predicate slots: windows / dwords -> R x u32 per slot */
        uint32_t lo[NS][R];
        #pragma unroll
        for (int s = 0; s < NS; s++)
            if ((uint32_t)s < nps) {
                if constexpr (WIN) ov_take<R>(c[s], crow, ww[s], fx[s], lo[s]);
                else ov_lows<R>(c[s], wn[s], lo[s]);
            }

        /* 2. next item's predicate windows / dwords, all slots back to back */
        const uint32_t it1 = it + G;
        const uint32_t nrow = (min(it1, last) % tpg) * TILE + lrow;
        uint32_t nw[NS][R];
        uint32_t nrows = 0;
        if constexpr (WIN) {
            /* straight into ww / fx: ov_take has read word 0 of every window */
            if (it1 < n_items && nrow < nrc) {
                #pragma unroll
                for (int s = 0; s < NS; s++)
                    if ((uint32_t)s < nps) ov_issue<R, false>(data, nc[s], nrow, ww[s], fx[s]);
            }
        } else {
            /* only the last tile of a group has rows past row_count to mask,
             * and an item that does not exist has no rows at all.
             * Into a fresh value per trip (zero where nothing is loaded), not
             * into wn: a dword that "keeps its old value" on some path is a
             * merge, and the merge a copy per dword per trip. The zeroes are
             * pinned here (empty asm) so that none is re-made between two
             * guarded loads, where writing the register would have to wait for
             * the loads in flight. */
            #pragma unroll
            for (int s = 0; s < NS; s++) {
                #pragma unroll
                for (int k = 0; k < R; k++) {
                    nw[s][k] = 0;
                    if ((uint32_t)s < nps) asm volatile("" : "+v"(nw[s][k]));
                }
            }
            if (it1 < n_items && nrow < nrc) nrows = ov_rows<R>(nrow, nrc);
            #pragma unroll
            for (int s = 0; s < NS; s++)
                if ((uint32_t)s < nps) ov_load<R>(data, nc[s], nrow, nrows, nw[s]);
            /* keep the scheduler from pulling a first use up between the loads */
            __builtin_amdgcn_sched_barrier(0);
        }

        /* 3. descriptors: ColLocs of item +2 (its GroupDesc came one trip
         * ago), GroupDesc of item +3 */
        OvRaw nn[NS] = {};
        #pragma unroll
        for (int s = 0; s < NS; s++)
            if ((uint32_t)s < ns) nn[s] = ov_fetch(colloc[g2.colbase + plan.slot_proj[s]]);
        const uint32_t nnrc = g2.row_count;
        const GroupDesc g3 = groups[min(it + 3u * G, last) / tpg];

        /* 4. every predicate from registers; row-pass flags as a bitmask */
        /* bit k = the lane's row k: crow + k (window form), crow +
         * k*AGG_BLOCK + t (lane form); set = the row lies inside the group */
        uint32_t pv = crows;
        if constexpr (WIN) {
            pv = 0;
            if (crow < crc) {
                const uint32_t left = crc - crow;
                pv = left >= (uint32_t)R ? (1u << R) - 1u : (1u << left) - 1u;
            }
        }
        uint32_t gv = 0;
        #pragma unroll
        for (uint32_t p = 0; p < (EXACT ? (uint32_t)NPREDS : n_preds); p++) {
            const uint32_t ctl = plan.pred_ctl[p];
            const int64_t ival = plan.pred_val[p];
            uint32_t o[R]; uint64_t h = 0;
            ov_pick<R, NS>(lo, c, EXACT ? (uint32_t)(SIG >> (2u * p)) & 3u
                                        : ctl & 0xFFu, o, h);
            const OvCmp cm = ov_cmp((ctl >> 8) & 0xFFu, h, ival);
            uint32_t g = 0;
            #pragma unroll
            for (int k = 0; k < R; k++)
                g |= (uint32_t)(o[k] - cm.a <= cm.d) << k;
            gv |= g ^ ((0u - cm.inv) & ((1u << R) - 1u));
            if (ctl >> 16) { pv &= gv; gv = 0; }
        }

        /* the wave-level test is the uniform branch round the whole fold;
         * inside it only the lanes that hold a passing row go on (pv != 0
         * implies the row exists): they alone load the operand-only slots,
         * so a 128-B line no passing lane reaches is never fetched, and a
         * lane with nothing to add folds nothing. */
        if (__ballot(pv != 0) != 0 && pv != 0) {
            if constexpr (WIN) {
                /* the lane's whole window, consumed at once */
                #pragma unroll
                for (int s = 0; s < NS; s++)
                    if ((uint32_t)s >= nps && (uint32_t)s < ns) {
                        uint64_t w[OV_NW(R)] = {};
                        uint32_t f = 0;
                        ov_issue<R, true>(data, c[s], crow, w, f);
                        ov_take<R>(c[s], crow, w, f, lo[s]);
                    }
            } else {
                /* only the lane's passing rows, so not even a line that no
                 * passing row lies in. All loads of all operand slots are
                 * issued into distinct registers first, then waited for
                 * once; a row that did not pass has a zero word, and every
                 * fold skips it anyway. */
                uint32_t ow[NS][R];
                #pragma unroll
                for (int s = 0; s < NS; s++) {
                    #pragma unroll
                    for (int k = 0; k < R; k++) ow[s][k] = 0;
                }
                #pragma unroll
                for (int s = 0; s < NS; s++)
                    if ((uint32_t)s >= nps && (uint32_t)s < ns)
                        ov_load<R>(data, c[s], crow, pv, ow[s]);
                __builtin_amdgcn_sched_barrier(0);
                #pragma unroll
                for (int s = 0; s < NS; s++)
                    if ((uint32_t)s >= nps && (uint32_t)s < ns)
                        ov_lows<R>(c[s], ow[s], lo[s]);
            }
            const int64_t cnt = __popc(pv);
            #pragma unroll
            for (int a = 0; a < NAGGS; a++) {
                if (!EXACT && (uint32_t)a >= n_aggs) continue;
                const AggD &g = params.aggs[a];
                uint32_t oa[R], ob[R], oc[R];
                uint64_t ha = 0, hb = 0, hc = 0;
                const uint32_t sa = EXACT ? (uint32_t)(SIG >> (32u + 6u * a)) & 3u
                                          : (uint32_t)plan.agg_slot[a][0];
                const uint32_t sb = EXACT ? (uint32_t)(SIG >> (34u + 6u * a)) & 3u
                                          : (uint32_t)plan.agg_slot[a][1];
                const uint32_t sc = EXACT ? (uint32_t)(SIG >> (36u + 6u * a)) & 3u
                                          : (uint32_t)plan.agg_slot[a][2];
                const uint32_t kind = EXACT ? (KSIG >> (4u * a)) & 15u : (uint32_t)g.kind;
                switch (kind) {                   /* values already in registers */
                    case CSTRIPE_AGG_COUNT_STAR:
                        acc[a].lo += cnt;
                        break;
                    case CSTRIPE_AGG_SUM_I64: {
                        ov_pick<R, NS>(lo, c, sa, oa, ha);
                        __int128 t = 0;
                        #pragma unroll
                        for (int k = 0; k < R; k++)
                            if ((pv >> k) & 1u) t += (__int128)ov_val(oa[k], ha);
                        acc_add_i128(acc[a], t);
                        break;
                    }
                    case CSTRIPE_AGG_MIN_I64:
                        ov_pick<R, NS>(lo, c, sa, oa, ha);
                        #pragma unroll
                        for (int k = 0; k < R; k++)
                            if ((pv >> k) & 1u) acc[a].lo = min(acc[a].lo, ov_val(oa[k], ha));
                        break;
                    case CSTRIPE_AGG_MAX_I64:
                        ov_pick<R, NS>(lo, c, sa, oa, ha);
                        #pragma unroll
                        for (int k = 0; k < R; k++)
                            if ((pv >> k) & 1u) acc[a].lo = max(acc[a].lo, ov_val(oa[k], ha));
                        break;
                    case CSTRIPE_AGG_SUM_PROD_I64: {
                        ov_pick<R, NS>(lo, c, sa, oa, ha);
                        ov_pick<R, NS>(lo, c, sb, ob, hb);
                        if (EXACT && (ha | hb) == 0 &&
                            __popc(ov_pick_mask<NS>(c, sa)) + __popc(ov_pick_mask<NS>(c, sb))
                                <= OV_NARROW_BITS) {
                            uint64_t u = 0;
                            #pragma unroll
                            for (int k = 0; k < R; k++)
                                u += (uint64_t)ov_sel(pv, k, oa[k]) * ob[k];
                            acc_add_i128(acc[a], (__int128)u);
                            break;
                        }
                        __int128 t = 0;
                        #pragma unroll
                        for (int k = 0; k < R; k++)
                            if ((pv >> k) & 1u)
                                t += (__int128)ov_val(oa[k], ha) * ov_val(ob[k], hb);
                        acc_add_i128(acc[a], t);
                        break;
                    }
                    case CSTRIPE_AGG_SUM_DISC_I64: {
                        ov_pick<R, NS>(lo, c, sa, oa, ha);
                        ov_pick<R, NS>(lo, c, sb, ob, hb);
                        __int128 t = 0;
                        #pragma unroll
                        for (int k = 0; k < R; k++)
                            if ((pv >> k) & 1u)
                                t += (__int128)ov_val(oa[k], ha) * (g.one - ov_val(ob[k], hb));
                        acc_add_i128(acc[a], t);
                        break;
                    }
                    case CSTRIPE_AGG_SUM_DISC_TAX_I64: {
                        ov_pick<R, NS>(lo, c, sa, oa, ha);
                        ov_pick<R, NS>(lo, c, sb, ob, hb);
                        ov_pick<R, NS>(lo, c, sc, oc, hc);
                        __int128 t = 0;
                        #pragma unroll
                        for (int k = 0; k < R; k++)
                            if ((pv >> k) & 1u)
                                t += (__int128)ov_val(oa[k], ha) * (g.one - ov_val(ob[k], hb))
                                     * (g.one + ov_val(oc[k], hc));
                        acc_add_i128(acc[a], t);
                        break;
                    }
                    default:
                        break;
                }
                acc[a].cnt += cnt;
            }
        }

        /* rotate the descriptor pipeline; the ColLocs fetched in (3) are
         * first touched here, a whole fold later */
        #pragma unroll
        for (int s = 0; s < NS; s++) {
            c[s] = nc[s]; nc[s] = ov_col(nn[s]);
            if constexpr (!WIN) {
                #pragma unroll
                for (int k = 0; k < R; k++) wn[s][k] = nw[s][k];
            }
        }
        crc = nrc; crow = nrow;
        if constexpr (!WIN) crows = nrows;
        nrc = nnrc;
        g2 = g3;
    }

    /* one wave/block reduce per block */
    block_reduce<NAGGS, true>(acc, params, n_aggs, block_out);
}

/* per-row precomputed aggregate contribution: operands loaded ONCE per row,
 * so the per-distinct-key reduce rounds touch registers only */
struct PrepAcc {
    int64_t lo, hi;    /* i128 contribution / i64 value */
    double f;
    bool valid;
};

__device__ inline void acc_prepare(PrepAcc &o, const AggD &g,
                                   const uint8_t *__restrict__ data,
                                   const uint8_t *__restrict__ scratch,
                                   const uint32_t *__restrict__ rank,
                                   const ColLoc *__restrict__ cols, uint32_t row)
{
    o.lo = 0; o.hi = 0; o.f = 0.0; o.valid = false;
    int64_t iv, ib, ic; double fv, fb, fc;
    switch (g.kind) {
        case CSTRIPE_AGG_COUNT_STAR:
            o.valid = true; o.lo = 1; break;
        case CSTRIPE_AGG_COUNT_COL:
            if (col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv)) { o.valid = true; o.lo = 1; }
            break;
        case CSTRIPE_AGG_SUM_I64:
        case CSTRIPE_AGG_MIN_I64:
        case CSTRIPE_AGG_MAX_I64:
            if (col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv)) {
                o.valid = true; o.lo = iv; o.hi = iv < 0 ? -1 : 0;
            }
            break;
        case CSTRIPE_AGG_SUM_F64:
        case CSTRIPE_AGG_MIN_F64:
        case CSTRIPE_AGG_MAX_F64:
            if (col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv)) { o.valid = true; o.f = fv; }
            break;
        case CSTRIPE_AGG_SUM_PROD_I64:
            if (col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv) &&
                col_value(data, scratch, rank, cols[g.proj_b], row, ib, fb)) {
                __int128 x = (__int128)iv * ib;
                o.valid = true; o.lo = (int64_t)(uint64_t)x; o.hi = (int64_t)(x >> 64);
            }
            break;
        case CSTRIPE_AGG_SUM_DISC_I64:
            if (col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv) &&
                col_value(data, scratch, rank, cols[g.proj_b], row, ib, fb)) {
                __int128 x = (__int128)iv * (g.one - ib);
                o.valid = true; o.lo = (int64_t)(uint64_t)x; o.hi = (int64_t)(x >> 64);
            }
            break;
        case CSTRIPE_AGG_SUM_DISC_TAX_I64:
            if (col_value(data, scratch, rank, cols[g.proj_a], row, iv, fv) &&
                col_value(data, scratch, rank, cols[g.proj_b], row, ib, fb) &&
                col_value(data, scratch, rank, cols[g.proj_c], row, ic, fc)) {
                __int128 x = (__int128)iv * (g.one - ib) * (g.one + ic);
                o.valid = true; o.lo = (int64_t)(uint64_t)x; o.hi = (int64_t)(x >> 64);
            }
            break;
    }
}


/* =====================================================================
 * Grouped aggregation (TPC-H Q1 shape): GROUP BY 1-2 categorical i8
 * columns, few distinct groups. The reference plan is worker HashAggregate
 * over ColumnarScan + coordinator merge per group (multi_explain.out:80-82,
 * multi_logical_optimizer.c:1807-1885). Here: per-WAVE LDS accumulator
 * tables (no atomics); rows reduce wave-cooperatively one distinct key at
 * a time (ballot + predicated identity + shuffle reduce); grid-stride
 * blocks flush one compact table each; a final single-block kernel merges.
 * ===================================================================== */

#define GRP_SLOTS CSTRIPE_MAX_GROUPS  /* distinct keys per wave table (a wave may see every group) */
#define GRP_GRID  1024        /* grid-stride blocks */

struct GroupParams {
    AggParams base;
    uint32_t n_group_cols;
    uint32_t gproj[CSTRIPE_MAX_GROUP_COLS];   /* projected slots of key cols */
    uint32_t n_work;                          /* n_groups * tiles_per_group */
};


/* fold a prepared contribution into an LDS accumulator cell with atomics —
 * per-lane, no wave-cooperative rounds. int128 sums stay EXACT: the carry of
 * my own low-half add is detected from atomicAdd's return value and added to
 * the high half (independent of interleaving). f64 sums become
 * atomic-order-dependent (covered by the 1e-6 float tolerance). */
__device__ inline void acc_apply_atomic(ThreadAcc *cell, uint8_t kind, const PrepAcc &p)
{
    if (!p.valid) return;
    switch (kind) {
        case CSTRIPE_AGG_MIN_I64:
            atomicMin((long long *)&cell->lo, (long long)p.lo);
            break;
        case CSTRIPE_AGG_MAX_I64:
            atomicMax((long long *)&cell->lo, (long long)p.lo);
            break;
        case CSTRIPE_AGG_MIN_F64: {
            double v = p.f;
            unsigned long long *addr = (unsigned long long *)&cell->f;
            unsigned long long cur = *addr;
            while (true) {
                double c;
                memcpy(&c, &cur, 8);
                if (f64cmp_pg(v, c) >= 0) break;   /* PG order (NaN high) */
                unsigned long long nv;
                memcpy(&nv, &v, 8);
                unsigned long long prev = atomicCAS(addr, cur, nv);
                if (prev == cur) break;
                cur = prev;
            }
            break;
        }
        case CSTRIPE_AGG_MAX_F64: {
            double v = p.f;
            unsigned long long *addr = (unsigned long long *)&cell->f;
            unsigned long long cur = *addr;
            while (true) {
                double c;
                memcpy(&c, &cur, 8);
                if (f64cmp_pg(v, c) <= 0) break;   /* PG order (NaN high) */
                unsigned long long nv;
                memcpy(&nv, &v, 8);
                unsigned long long prev = atomicCAS(addr, cur, nv);
                if (prev == cur) break;
                cur = prev;
            }
            break;
        }
        case CSTRIPE_AGG_SUM_F64:
            atomicAdd((double *)&cell->f, p.f);
            break;
        default: {   /* counts + i128 sums */
            unsigned long long old =
                atomicAdd((unsigned long long *)&cell->lo, (unsigned long long)p.lo);
            int64_t carry = (old + (unsigned long long)p.lo) < old ? 1 : 0;
            int64_t hi = p.hi + carry;
            if (hi) atomicAdd((unsigned long long *)&cell->hi, (unsigned long long)hi);
            break;
        }
    }
    atomicAdd((unsigned long long *)&cell->cnt, 1ull);
}

/* =====================================================================
 * Multi-row GROUPED kernel for ALL-DENSE chunks (TPC-H Q1 shape): the same
 * R-row windowed loads as multi_agg_kernel (the scan is load-latency
 * bound), folding into a per-WAVE 16-slot LDS group table with the
 * carry-exact atomics. >16 distinct keys set device flag 8 and the host
 * re-runs the 64-group fallback (grouped_agg_kernel).
 * ===================================================================== */

#define MGRP_SLOTS 16

/* value-only LDS fold: multi_grouped tracks ONE per-slot row counter (all
 * operands are dense there, so every agg's count equals the group's row
 * count) — halves the per-row LDS atomic traffic vs acc_apply_atomic */
__device__ inline void acc_apply_value_atomic(ThreadAcc *cell, uint8_t kind,
                                              const PrepAcc &p)
{
    switch (kind) {
        case CSTRIPE_AGG_COUNT_STAR:
        case CSTRIPE_AGG_COUNT_COL:
            return;                         /* derived from the slot counter */
        case CSTRIPE_AGG_MIN_I64:
            atomicMin((long long *)&cell->lo, (long long)p.lo);
            return;
        case CSTRIPE_AGG_MAX_I64:
            atomicMax((long long *)&cell->lo, (long long)p.lo);
            return;
        case CSTRIPE_AGG_SUM_F64:
            atomicAdd((double *)&cell->f, p.f);
            return;
        case CSTRIPE_AGG_MIN_F64:
        case CSTRIPE_AGG_MAX_F64: {
            unsigned long long *addr = (unsigned long long *)&cell->f;
            unsigned long long cur = *addr;
            const bool want_min = kind == CSTRIPE_AGG_MIN_F64;
            while (true) {
                double c;
                memcpy(&c, &cur, 8);
                const int cmp = f64cmp_pg(p.f, c);
                if (want_min ? cmp >= 0 : cmp <= 0) break;
                unsigned long long nv;
                memcpy(&nv, &p.f, 8);
                unsigned long long prev = atomicCAS(addr, cur, nv);
                if (prev == cur) break;
                cur = prev;
            }
            return;
        }
        default: {                          /* i128 sums, carry-exact */
            unsigned long long old =
                atomicAdd((unsigned long long *)&cell->lo, (unsigned long long)p.lo);
            int64_t carry = (old + (unsigned long long)p.lo) < old ? 1 : 0;
            int64_t hi = p.hi + carry;
            if (hi) atomicAdd((unsigned long long *)&cell->hi, (unsigned long long)hi);
            return;
        }
    }
}

template <int NAGGS, int R>
__global__ __launch_bounds__(AGG_BLOCK, 4) void multi_grouped_kernel(
    const uint8_t *__restrict__ data, const uint8_t *__restrict__ scratch,
    const GroupDesc *__restrict__ groups, const ColLoc *__restrict__ colloc,
    uint32_t *__restrict__ keys_out, AccCell *__restrict__ cells_out,
    int *__restrict__ err, const GroupParams gp)
{
    const AggParams &params = gp.base;
    const uint32_t n_aggs = NAGGS >= 0 ? (uint32_t)NAGGS : params.n_aggs;
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t n_waves = AGG_BLOCK / WAVE;
    constexpr uint32_t HALF = (uint32_t)R * AGG_BLOCK;   /* rows per pass */

    __shared__ int wkeys[AGG_BLOCK / WAVE][MGRP_SLOTS];
    __shared__ unsigned long long wcnt[AGG_BLOCK / WAVE][MGRP_SLOTS];
    extern __shared__ uint8_t mg_lds[];
    ThreadAcc *wacc = (ThreadAcc *)mg_lds;   /* [wave][slot][agg] */

    for (uint32_t i = threadIdx.x; i < n_waves * MGRP_SLOTS; i += AGG_BLOCK) {
        wkeys[i / MGRP_SLOTS][i % MGRP_SLOTS] = -1;
        wcnt[i / MGRP_SLOTS][i % MGRP_SLOTS] = 0;
        for (uint32_t a = 0; a < n_aggs; a++)
            acc_init(wacc[i * n_aggs + a], params.aggs[a].kind);
    }
    __syncthreads();

    ThreadAcc *myacc = wacc + (size_t)wid * MGRP_SLOTS * n_aggs;
    int *mykeys = wkeys[wid];
    unsigned long long *mycnt = wcnt[wid];
    uint32_t ck0 = ~0u, ck1 = ~0u, cs0 = 0, cs1 = 0;   /* key->slot cache */

    /* grid-stride over (chunk, tile) work items: tables persist across
     * items and flush once, keeping per-block output buffers small */
    for (uint32_t work = blockIdx.x; work < gp.n_work; work += gridDim.x) {
    const uint32_t gid = work / params.tiles_per_group;
    const uint32_t tile = work % params.tiles_per_group;
    const GroupDesc g = groups[gid];
    const ColLoc *cols = colloc + g.colbase;
    const uint32_t row_start = tile * TILE_ROWS;
    const uint32_t row_end = min(row_start + TILE_ROWS, g.row_count);

    for (uint32_t half_start = row_start; half_start < row_end;
         half_start += HALF) {
        const uint32_t half_end = min(half_start + HALF, row_end);
        const uint32_t my0 = half_start + R * threadIdx.x;
        bool pv[R], gv[R];
        #pragma unroll
        for (int k = 0; k < R; k++) { pv[k] = my0 + k < half_end; gv[k] = false; }
        int last_proj = -1;
        ValsR<R> q{};
        #pragma unroll
        for (uint32_t pp = 0; pp < params.n_preds; pp++) {
            const PredD &pr = params.preds[pp];
            if ((int)pr.proj != last_proj) {
                col_multi<R>(data, scratch, cols[pr.proj],
                             my0 < half_end ? my0 : half_start, q);
                last_proj = (int)pr.proj;
            }
            #pragma unroll
            for (int k = 0; k < R; k++)
                gv[k] = gv[k] | pred_eval(pr, q.v[k], q.fget(k));
            if (pr.gend) {
                #pragma unroll
                for (int k = 0; k < R; k++) { pv[k] = pv[k] & gv[k]; gv[k] = false; }
                /* early wave exit after a dead AND-group (see multi_agg) */
                bool alive = false;
                #pragma unroll
                for (int k = 0; k < R; k++) alive |= pv[k];
                if (__ballot(alive) == 0) break;
            }
        }
        bool any = false;
        #pragma unroll
        for (int k = 0; k < R; k++) any |= pv[k];
        if (__ballot(any) != 0) {

        /* group keys through col_multi; 9-bit enc (bit 8 = NULL never set:
         * dense) */
        uint32_t key[R];
        {
            const uint32_t safe0 = my0 < half_end ? my0 : half_start;
            #pragma unroll
            for (int k = 0; k < R; k++) key[k] = 0;
            for (uint32_t i = 0; i < gp.n_group_cols; i++) {
                const uint32_t pj = gp.gproj[i];
                const bool is_text = cols[pj].type == CSTRIPE_TEXT;
                ValsR<R> kq;
                col_multi<R>(data, scratch, cols[pj], safe0, kq);
                #pragma unroll
                for (int k = 0; k < R; k++) {
                    uint32_t raw = (uint32_t)kq.v[k];
                    if (is_text) raw >>= 8;
                    key[k] |= (raw & 0xFF) << (9 * i);
                }
            }
        }
        /* slot per row: register cache, else LDS claim (CAS linear probe) */
        uint32_t slot[R];
        #pragma unroll
        for (int k = 0; k < R; k++) {
            slot[k] = 0xFFFFFFFF;
            if (!pv[k]) continue;
            if (key[k] == ck0) slot[k] = cs0;
            else if (key[k] == ck1) slot[k] = cs1;
            else {
                for (uint32_t s2 = 0; s2 < MGRP_SLOTS; s2++) {
                    int old = atomicCAS(&mykeys[s2], -1, (int)key[k]);
                    if (old == -1 || old == (int)key[k]) { slot[k] = s2; break; }
                }
                if (slot[k] == 0xFFFFFFFF) { atomicOr(err, 8); pv[k] = false; continue; }
                ck1 = ck0; cs1 = cs0;
                ck0 = key[k]; cs0 = slot[k];
            }
        }

        /* one row counter per slot (dense: every agg's count equals it) */
        #pragma unroll
        for (int k = 0; k < R; k++)
            if (pv[k]) atomicAdd(&mycnt[slot[k]], 1ull);

        /* operand loads once per agg column, contributions folded per row */
        const uint32_t safe0 = my0 < half_end ? my0 : half_start;
        #pragma unroll
        for (uint32_t a = 0; a < n_aggs; a++) {
            const AggD &ag = params.aggs[a];
            const uint8_t kind = ag.kind;
            ValsR<R> qa, qb, qc;
            if (kind != CSTRIPE_AGG_COUNT_STAR && kind != CSTRIPE_AGG_COUNT_COL) {
                col_multi<R>(data, scratch, cols[ag.proj_a], safe0, qa);
                if (kind >= CSTRIPE_AGG_SUM_PROD_I64)
                    col_multi<R>(data, scratch, cols[ag.proj_b], safe0, qb);
                if (kind == CSTRIPE_AGG_SUM_DISC_TAX_I64)
                    col_multi<R>(data, scratch, cols[ag.proj_c], safe0, qc);
            }
            #pragma unroll
            for (int k = 0; k < R; k++) {
                if (!pv[k]) continue;
                PrepAcc pc;
                pc.valid = true; pc.f = 0.0; pc.lo = 0; pc.hi = 0;
                switch (kind) {
                    case CSTRIPE_AGG_COUNT_STAR:
                    case CSTRIPE_AGG_COUNT_COL: pc.lo = 1; break;
                    case CSTRIPE_AGG_SUM_I64:
                    case CSTRIPE_AGG_MIN_I64:
                    case CSTRIPE_AGG_MAX_I64:
                        pc.lo = qa.v[k]; pc.hi = qa.v[k] < 0 ? -1 : 0; break;
                    case CSTRIPE_AGG_SUM_F64:
                    case CSTRIPE_AGG_MIN_F64:
                    case CSTRIPE_AGG_MAX_F64:
                        pc.f = qa.fget(k); break;
                    case CSTRIPE_AGG_SUM_PROD_I64: {
                        __int128 x = (__int128)qa.v[k] * qb.v[k];
                        pc.lo = (int64_t)(uint64_t)x; pc.hi = (int64_t)(x >> 64); break;
                    }
                    case CSTRIPE_AGG_SUM_DISC_I64: {
                        __int128 x = (__int128)qa.v[k] * (ag.one - qb.v[k]);
                        pc.lo = (int64_t)(uint64_t)x; pc.hi = (int64_t)(x >> 64); break;
                    }
                    case CSTRIPE_AGG_SUM_DISC_TAX_I64: {
                        __int128 x = (__int128)qa.v[k] * (ag.one - qb.v[k])
                                     * (ag.one + qc.v[k]);
                        pc.lo = (int64_t)(uint64_t)x; pc.hi = (int64_t)(x >> 64); break;
                    }
                    default: pc.valid = false; break;
                }
                acc_apply_value_atomic(&myacc[slot[k] * n_aggs + a], kind, pc);
            }
        }
        }   /* wave has passing rows */
    }   /* half loop */
    }   /* work loop */
    __syncthreads();

    /* merge the block's wave tables into one compact list (as grouped_agg) */
    if (threadIdx.x == 0) {
        uint32_t *bk = keys_out + (size_t)blockIdx.x * (n_waves * MGRP_SLOTS);
        AccCell *bc = cells_out + (size_t)blockIdx.x * (n_waves * MGRP_SLOTS) * n_aggs;
        uint32_t n = 0;
        for (uint32_t w = 0; w < n_waves; w++) {
            for (uint32_t s2 = 0; s2 < MGRP_SLOTS; s2++) {
                int kk = wkeys[w][s2];
                if (kk < 0) continue;
                uint32_t at = n;
                for (uint32_t j = 0; j < n; j++) if (bk[j] == (uint32_t)kk) { at = j; break; }
                ThreadAcc *src = wacc + ((size_t)(w * MGRP_SLOTS) + s2) * n_aggs;
                const int64_t rowcnt = (int64_t)wcnt[w][s2];
                for (uint32_t a = 0; a < n_aggs; a++) {
                    src[a].cnt = rowcnt;
                    const uint8_t kd = params.aggs[a].kind;
                    if (kd == CSTRIPE_AGG_COUNT_STAR || kd == CSTRIPE_AGG_COUNT_COL)
                        src[a].lo = rowcnt;
                }
                if (at == n) {
                    bk[n] = (uint32_t)kk;
                    for (uint32_t a = 0; a < n_aggs; a++) {
                        AccCell c{src[a].lo, src[a].hi, src[a].f, src[a].cnt};
                        bc[(size_t)n * n_aggs + a] = c;
                    }
                    n++;
                } else {
                    for (uint32_t a = 0; a < n_aggs; a++) {
                        AccCell c = bc[(size_t)at * n_aggs + a];
                        ThreadAcc cur{c.lo, c.hi, c.f, c.cnt};
                        acc_merge(cur, src[a], params.aggs[a].kind);
                        AccCell o{cur.lo, cur.hi, cur.f, cur.cnt};
                        bc[(size_t)at * n_aggs + a] = o;
                    }
                }
            }
        }
        for (uint32_t j = n; j < n_waves * MGRP_SLOTS; j++) bk[j] = 0xFFFFFFFFu;
    }
}

template <int NAGGS>
__global__ __launch_bounds__(AGG_BLOCK) void grouped_agg_kernel(
    const uint8_t *__restrict__ data, const uint8_t *__restrict__ scratch,
    const uint32_t *__restrict__ rank, const GroupDesc *__restrict__ groups,
    const ColLoc *__restrict__ colloc, uint32_t *__restrict__ keys_out,
    AccCell *__restrict__ cells_out, int *__restrict__ err,
    const GroupParams gp)
{
    const AggParams &params = gp.base;
    /* compile-time agg count unrolls the prep/reduce loops so the per-row
     * PrepAcc array stays in registers instead of scratch */
    const uint32_t n_aggs_ct = NAGGS >= 0 ? (uint32_t)NAGGS : params.n_aggs;
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t n_waves = AGG_BLOCK / WAVE;

    extern __shared__ uint8_t gsh[];
    uint32_t *wkeys = (uint32_t *)gsh;                          /* [wave][S] */
    ThreadAcc *wacc = (ThreadAcc *)(gsh + n_waves * GRP_SLOTS * sizeof(uint32_t));
    /* wacc[((wave*S)+slot)*n_aggs + a] */

    for (uint32_t i = threadIdx.x; i < n_waves * GRP_SLOTS; i += AGG_BLOCK)
        wkeys[i] = 0xFFFFFFFFu;
    __syncthreads();

    uint32_t *mykeys = wkeys + wid * GRP_SLOTS;
    ThreadAcc *myacc = wacc + (size_t)wid * GRP_SLOTS * n_aggs_ct;
    uint32_t used = 0;       /* wave-uniform slot count (updated by lane 0 path) */
    /* per-lane 4-way key->slot register cache: hits skip the wave-ballot
     * slot rounds entirely (few distinct groups => near-100% after warmup) */
    uint32_t ck0 = ~0u, ck1 = ~0u, ck2 = ~0u, ck3 = ~0u;
    uint32_t cs0 = 0, cs1 = 0, cs2 = 0, cs3 = 0;

    for (uint32_t work = blockIdx.x; work < gp.n_work; work += gridDim.x) {
        const uint32_t gid = work / params.tiles_per_group;
        const uint32_t tile = work % params.tiles_per_group;
        const GroupDesc g = groups[gid];
        const ColLoc *cols = colloc + g.colbase;
        uint32_t row_start = tile * TILE_ROWS;
        uint32_t row_end = min(row_start + TILE_ROWS, g.row_count);

        for (uint32_t base_row = row_start + wid * WAVE; base_row < row_end;
             base_row += WAVE * n_waves) {
            uint32_t row = base_row + lane;
            bool pass = row < row_end;
            if (pass) {
                int last_proj = -1;
                int64_t liv = 0; double lfv = 0; bool lok = false;
                bool gv = false;
                for (uint32_t p = 0; p < params.n_preds; p++) {
                    const PredD &pr = params.preds[p];
                    if ((int)pr.proj != last_proj) {
                        lok = col_value(data, scratch, rank, cols[pr.proj], row, liv, lfv);
                        last_proj = (int)pr.proj;
                    }
                    gv = gv | (lok && pred_eval(pr, liv, lfv));
                    if (pr.gend) { pass = pass & gv; gv = false; }
                }
            }
            uint32_t key = 0;
            if (pass) {
                int64_t kv; double kf;
                for (uint32_t gc = 0; gc < gp.n_group_cols; gc++) {
                    /* NULL keys form their own group (reference
                     * HashAggregate treats NULLs as equal): 9-bit encoding,
                     * bit 8 = null. TEXT keys group by the first payload
                     * byte of the varlena slot (char(1) semantics). */
                    const ColLoc &kc = cols[gp.gproj[gc]];
                    bool ok = col_value(data, scratch, rank, kc, row, kv, kf);
                    uint32_t raw = (uint32_t)kv;
                    if (kc.type == CSTRIPE_TEXT) raw >>= 8;
                    uint32_t enc = ok ? (raw & 0xFF) : CSTRIPE_GROUP_KEY_NULL;
                    key |= enc << (9 * gc);
                }
            }
            /* round 0 (agg-independent): assign each passing lane its key's
             * wave-table slot — register cache first, ballot rounds only
             * for misses */
            uint32_t myslot = 0xFFFFFFFF;
            if (pass) {
                if (key == ck0) myslot = cs0;
                else if (key == ck1) myslot = cs1;
                else if (key == ck2) myslot = cs2;
                else if (key == ck3) myslot = cs3;
            }
            {
                uint64_t remaining = __ballot(pass && myslot == 0xFFFFFFFF);
                while (remaining) {
                    int leader = __ffsll((unsigned long long)remaining) - 1;
                    uint32_t kk = (uint32_t)__shfl((int)key, leader, WAVE);
                    bool mine = pass && key == kk;
                    uint32_t slot = 0xFFFFFFFF;
                    for (uint32_t sidx = 0; sidx < used; sidx++)
                        if (mykeys[sidx] == kk) { slot = sidx; break; }
                    if (slot == 0xFFFFFFFF) {
                        if (used >= GRP_SLOTS) {      /* overflow: flag + drop */
                            if (lane == 0) atomicOr(err, 8);
                            remaining &= ~__ballot(mine);
                            continue;
                        }
                        slot = used++;
                        if (lane == 0) mykeys[slot] = kk;
                        for (uint32_t a = 0; a < n_aggs_ct; a++) {
                            ThreadAcc z;
                            acc_init(z, params.aggs[a].kind);
                            if (lane == 0) myacc[slot * n_aggs_ct + a] = z;
                        }
                    }
                    if (mine) {
                        myslot = slot;
                        ck3 = ck2; cs3 = cs2;
                        ck2 = ck1; cs2 = cs1;
                        ck1 = ck0; cs1 = cs0;
                        ck0 = key; cs0 = slot;
                    }
                    remaining &= ~__ballot(mine);
                }
            }
            /* per agg (unrolled): one prepared contribution per row folded
             * into the wave's LDS table with per-lane atomics */
            if (pass && myslot != 0xFFFFFFFF) {
                for (uint32_t a = 0; a < n_aggs_ct; a++) {
                    PrepAcc p;
                    acc_prepare(p, params.aggs[a], data, scratch, rank, cols, row);
                    acc_apply_atomic(&myacc[myslot * n_aggs_ct + a],
                                     params.aggs[a].kind, p);
                }
            }
        }
    }
    __syncthreads();

    /* merge the block's wave tables into one compact list; write to global.
     * wave 0 lane 0 does it serially — tables are tiny. */
    if (threadIdx.x == 0) {
        uint32_t *bk = keys_out + (size_t)blockIdx.x * (n_waves * GRP_SLOTS);
        AccCell *bc = cells_out + (size_t)blockIdx.x * (n_waves * GRP_SLOTS) * n_aggs_ct;
        uint32_t n = 0;
        for (uint32_t w = 0; w < n_waves; w++) {
            for (uint32_t sidx = 0; sidx < GRP_SLOTS; sidx++) {
                uint32_t k = wkeys[w * GRP_SLOTS + sidx];
                if (k == 0xFFFFFFFFu) continue;
                uint32_t at = n;
                for (uint32_t j = 0; j < n; j++) if (bk[j] == k) { at = j; break; }
                ThreadAcc *src = wacc + ((size_t)(w * GRP_SLOTS) + sidx) * n_aggs_ct;
                if (at == n) {
                    bk[n] = k;
                    for (uint32_t a = 0; a < n_aggs_ct; a++) {
                        AccCell c{src[a].lo, src[a].hi, src[a].f, src[a].cnt};
                        bc[(size_t)n * n_aggs_ct + a] = c;
                    }
                    n++;
                } else {
                    for (uint32_t a = 0; a < n_aggs_ct; a++) {
                        AccCell c = bc[(size_t)at * n_aggs_ct + a];
                        ThreadAcc cur{c.lo, c.hi, c.f, c.cnt};
                        acc_merge(cur, src[a], params.aggs[a].kind);
                        AccCell o{cur.lo, cur.hi, cur.f, cur.cnt};
                        bc[(size_t)at * n_aggs_ct + a] = o;
                    }
                }
            }
        }
        for (uint32_t j = n; j < n_waves * GRP_SLOTS; j++) bk[j] = 0xFFFFFFFFu;
    }
}

/* single-block merge of per-block group tables -> final <=64 groups.
 * Parallel: 256 threads stride the (block, slot) entries; keys claim final
 * slots via LDS CAS (linear probe); cells merge with the same atomic
 * carry-exact machinery as the main kernel. */
__device__ inline void cell_merge_atomic(ThreadAcc *dst, uint8_t kind, const AccCell &src)
{
    switch (kind) {
        case CSTRIPE_AGG_MIN_I64:
            atomicMin((long long *)&dst->lo, (long long)src.lo);
            break;
        case CSTRIPE_AGG_MAX_I64:
            atomicMax((long long *)&dst->lo, (long long)src.lo);
            break;
        case CSTRIPE_AGG_MIN_F64: {
            unsigned long long *addr = (unsigned long long *)&dst->f;
            unsigned long long cur = *addr;
            while (true) {
                double c;
                memcpy(&c, &cur, 8);
                if (f64cmp_pg(src.f, c) >= 0) break;   /* PG order (NaN high) */
                unsigned long long nv;
                memcpy(&nv, &src.f, 8);
                unsigned long long prev = atomicCAS(addr, cur, nv);
                if (prev == cur) break;
                cur = prev;
            }
            break;
        }
        case CSTRIPE_AGG_MAX_F64: {
            unsigned long long *addr = (unsigned long long *)&dst->f;
            unsigned long long cur = *addr;
            while (true) {
                double c;
                memcpy(&c, &cur, 8);
                if (f64cmp_pg(src.f, c) <= 0) break;   /* PG order (NaN high) */
                unsigned long long nv;
                memcpy(&nv, &src.f, 8);
                unsigned long long prev = atomicCAS(addr, cur, nv);
                if (prev == cur) break;
                cur = prev;
            }
            break;
        }
        case CSTRIPE_AGG_SUM_F64:
            atomicAdd((double *)&dst->f, src.f);
            break;
        default: {
            unsigned long long old =
                atomicAdd((unsigned long long *)&dst->lo, (unsigned long long)src.lo);
            int64_t carry = (old + (unsigned long long)src.lo) < old ? 1 : 0;
            int64_t hi = src.hi + carry;
            if (hi) atomicAdd((unsigned long long *)&dst->hi, (unsigned long long)hi);
            break;
        }
    }
    atomicAdd((unsigned long long *)&dst->cnt, (unsigned long long)src.cnt);
}

__global__ __launch_bounds__(AGG_BLOCK) void grouped_final_kernel(
    const uint32_t *__restrict__ keys_in, const AccCell *__restrict__ cells_in,
    uint32_t n_blocks, uint32_t per_block, uint32_t *__restrict__ keys_out,
    AccCell *__restrict__ cells_out, uint32_t *__restrict__ n_groups_out,
    int *__restrict__ err, const GroupParams gp)
{
    const AggParams &params = gp.base;
    __shared__ int skeys[CSTRIPE_MAX_GROUPS];
    __shared__ ThreadAcc scells[CSTRIPE_MAX_GROUPS * MAX_AGGS];
    for (uint32_t i = threadIdx.x; i < CSTRIPE_MAX_GROUPS; i += AGG_BLOCK) {
        skeys[i] = -1;
        for (uint32_t a = 0; a < params.n_aggs; a++)
            acc_init(scells[i * MAX_AGGS + a], params.aggs[a].kind);
    }
    __syncthreads();

    const uint32_t total = n_blocks * per_block;
    for (uint32_t f = threadIdx.x; f < total; f += AGG_BLOCK) {
        uint32_t k = keys_in[f];
        if (k == 0xFFFFFFFFu) continue;
        int slot = -1;
        for (uint32_t s = 0; s < CSTRIPE_MAX_GROUPS; s++) {
            int old = atomicCAS(&skeys[s], -1, (int)k);
            if (old == -1 || old == (int)k) { slot = (int)s; break; }
        }
        if (slot < 0) { atomicOr(err, 16); continue; }
        const AccCell *src = cells_in + (size_t)f * params.n_aggs;
        for (uint32_t a = 0; a < params.n_aggs; a++)
            cell_merge_atomic(&scells[slot * MAX_AGGS + a], params.aggs[a].kind, src[a]);
    }
    __syncthreads();

    if (threadIdx.x == 0) {
        uint32_t n = 0;
        for (uint32_t s = 0; s < CSTRIPE_MAX_GROUPS; s++) {
            if (skeys[s] < 0) continue;
            keys_out[n] = (uint32_t)skeys[s];
            for (uint32_t a = 0; a < params.n_aggs; a++) {
                const ThreadAcc &t = scells[s * MAX_AGGS + a];
                AccCell c{t.lo, t.hi, t.f, t.cnt};
                cells_out[(size_t)n * params.n_aggs + a] = c;
            }
            n++;
        }
        *n_groups_out = n;
    }
}

/* device-wide reduce over block partials; each launched block reduces a
 * grid-strided slice into out[blockIdx * n_aggs + a]. Large grids (1B-row
 * scans emit ~300k block partials) run this twice: wide pass then a
 * single-block pass over the wide pass's outputs. */
__global__ __launch_bounds__(AGG_BLOCK) void final_reduce_kernel(
    const AccCell *__restrict__ block_in, uint32_t n_blocks,
    AccCell *__restrict__ out, const AggParams params)
{
    __shared__ ThreadAcc lds[AGG_BLOCK / WAVE][MAX_AGGS];
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    for (uint32_t a = 0; a < params.n_aggs; a++) {
        ThreadAcc r;
        acc_init(r, params.aggs[a].kind);
        for (uint64_t b = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x;
             b < n_blocks; b += (uint64_t)gridDim.x * AGG_BLOCK) {
            const AccCell c = block_in[b * params.n_aggs + a];
            ThreadAcc t{c.lo, c.hi, c.f, c.cnt};
            acc_merge(r, t, params.aggs[a].kind);
        }
        wave_reduce(r, params.aggs[a].kind);
        if (lane == 0) lds[wid][a] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            ThreadAcc f = lds[0][a];
            for (uint32_t w = 1; w < AGG_BLOCK / WAVE; w++)
                acc_merge(f, lds[w][a], params.aggs[a].kind);
            AccCell c{f.lo, f.hi, f.f, f.cnt};
            out[(uint64_t)blockIdx.x * params.n_aggs + a] = c;
        }
        __syncthreads();
    }
}

#define FINAL_WIDE_GRID 240

/* launch the (possibly two-stage) final reduce: d_block[n_blocks] -> d_final */
static int launch_final_reduce(cs_gpu_state *g, uint32_t n_blocks,
                               const AggParams &p)
{
    if (n_blocks > 8192) {
        hipLaunchKernelGGL(final_reduce_kernel, dim3(FINAL_WIDE_GRID),
                           dim3(AGG_BLOCK), 0, g->stream,
                           g->d_block, n_blocks, g->d_final2, p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(final_reduce_kernel, dim3(1), dim3(AGG_BLOCK), 0,
                           g->stream, g->d_final2, FINAL_WIDE_GRID, g->d_final, p);
        HIP_TRY(hipGetLastError());
    } else {
        hipLaunchKernelGGL(final_reduce_kernel, dim3(1), dim3(AGG_BLOCK), 0,
                           g->stream, g->d_block, n_blocks, g->d_final, p);
        HIP_TRY(hipGetLastError());
    }
    return CSTRIPE_OK;
}

/* closed-form decode of ONE canonical segment to a dense value buffer —
 * used by the batch/parity path (next_batch) for canonical chunks, which
 * the agg kernels never materialize. One thread per value; coalesced
 * stores; the "decode" is just the canonical position formula (format.h). */
__global__ void canon_decode_kernel(const uint8_t *__restrict__ src,
                                    uint8_t *__restrict__ dst,
                                    uint32_t n_values, uint32_t mode,
                                    uint32_t L, uint32_t width, uint64_t hval)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_values) return;
    if (mode == CSF_SEGMODE_LIT) {
        const uint8_t *s = src + hval + (uint64_t)i * width;
        uint8_t *d = dst + (uint64_t)i * width;
        for (uint32_t j = 0; j < width; j++) d[j] = s[j];
        return;
    }
    if ((mode & 0xF8u) == CSF_SEGMODE_ZR4B_BASE) {      /* width-4 slots */
        uint32_t slot = (uint32_t)hval;
        if (mode != CSF_SEGMODE_ZR4_CONST) {
            const uint32_t pos = 15u + (i == 0 ? L : i + 3u + L);
            slot |= (uint32_t)src[pos] << (8u * L);
        }
        *(uint32_t *)(dst + (uint64_t)i * 4) = slot;
        return;
    }
    uint64_t v;
    if (mode == CSF_SEGMODE_CONST || mode == CSF_SEGMODE_ZR_CONST) {
        v = hval;
    } else {
        const uint32_t pos = canon_pos((uint8_t)mode, L, i);
        uint64_t lo;
        __builtin_memcpy(&lo, src + pos, 8);
        const uint64_t m = (~0ull) >> ((8u - L) * 8u);
        v = (lo & m) | hval;
    }
    *(uint64_t *)(dst + (uint64_t)i * 8) = v;
}

/* restricted-zstd decode: ONE LANE per frame segment. The frames are this
 * writer's own emission (raw literals + predefined-FSE sequences,
 * zstd_r.h), so the decoder needs no per-frame table build — the three
 * spec-fixed FSE tables are staged once. Output goes straight to scratch;
 * the agg kernels then read it like any decoded stream, so zstd timed
 * regions INCLUDE decompression on device (round-1 VERDICT #4). */
__global__ void zr_decode_kernel(const uint8_t *__restrict__ data,
                                 uint8_t *__restrict__ scratch,
                                 const SegDesc *__restrict__ segs, uint32_t n,
                                 const zr_dtables *__restrict__ dt,
                                 int *__restrict__ err)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SegDesc s = segs[i];
    const int r = zr_decode_frame(data + s.src_off, (int)s.comp_len,
                                  scratch + s.dst_off, (int)s.decomp_len,
                                  dt->ll, dt->ml, dt->of);
    if (r != (int)s.decomp_len) atomicOr(err, 32);
}

/* ---- device-tuned restricted-frame decoder -----------------------------
 * Same algorithm as zstd_r.h zr_decode_frame (which stays the host decoder
 * and the spec reference — parity is pinned lane-for-lane by the GPU
 * tests), restated for a 4-BYTE-ALIGNED LDS-resident frame. The reason it
 * exists: ds_read/ds_write require natural alignment, so every unaligned
 * 8-byte memcpy in the shared decoder compiles to EIGHT ds_read_u8 ops on
 * the serial FSE chain. Here every LDS access is an aligned dword:
 *  - bit-window refill = two ds_read_b32 (frame base is 4-aligned and the
 *    LDS stride leaves >= 8 B slack, so the aligned window may run past
 *    comp_len into the lane's own slack — those junk bits sit above the
 *    marker bit and are never returned);
 *  - FSE cell fetch = one ds_read_b32 (cells are 4 B);
 *  - literal reads = funnel over aligned dwords.
 * Global-memory accesses (decoded output, match copies) keep unaligned
 * 8-byte memcpys — gfx950 global/flat loads are alignment-tolerant and
 * already compile to dwordx2. */
struct zr_brd {
    const uint8_t *src;    /* 4-aligned LDS frame base */
    int32_t bitpos;
    int32_t wbase;         /* 4-aligned byte index of window LSB (-1 empty) */
    uint64_t w;
};

__device__ inline uint32_t zr_lds_u32(const uint8_t *p)   /* p 4-aligned */
{
    return *(const uint32_t *)__builtin_assume_aligned(p, 4);
}

__device__ inline int zr_brd_init(zr_brd *b, const uint8_t *src, int len)
{
    b->src = src;
    b->wbase = -1;
    b->w = 0;
    int last = len - 1;
    while (last >= 0 && src[last] == 0) last--;
    if (last < 0) return -1;
    int hb = 7;
    while (!(src[last] & (1 << hb))) hb--;
    b->bitpos = last * 8 + hb;
    return 0;
}

__device__ inline uint32_t zr_brd_read(zr_brd *b, int nbits)
{
    if (nbits == 0) return 0;
    b->bitpos -= nbits;
    const int32_t bp = b->bitpos < 0 ? 0 : b->bitpos;
    const int32_t byte = bp >> 3;
    if (b->wbase < 0 || byte < b->wbase || (bp - b->wbase * 8) + nbits > 64) {
        int32_t base = (byte - 2) & ~3;     /* byte-base in [2,5] -> any
                                             * <=16-bit read fits the window */
        if (base < 0) base = 0;
        b->w = (uint64_t)zr_lds_u32(b->src + base) |
               ((uint64_t)zr_lds_u32(b->src + base + 4) << 32);
        b->wbase = base;
    }
    const int32_t sh = bp - b->wbase * 8;
    return (uint32_t)(b->w >> sh) & ((1u << nbits) - 1u);
}

/* one 4-byte FSE cell as a single dword: sym | nbits<<8 | base<<16 */
__device__ inline uint32_t zr_cell_d(const zr_dcell *t, uint32_t s)
{
    return *(const uint32_t *)__builtin_assume_aligned(t + s, 4);
}

/* copy n bytes from the LDS frame (arbitrary offset so, frame base
 * 4-aligned with slack) to global dst: aligned-dword funnel loads,
 * unaligned 8-byte global stores */
__device__ inline void zr_lds_copy(uint8_t *dst, const uint8_t *src4,
                                   uint32_t so, uint32_t n)
{
    const uint32_t mis = so & 3u;
    const uint8_t *al = src4 + (so & ~3u);
    uint32_t i = 0;
    if (n >= 8) {
        const uint32_t sh = mis * 8u;
        uint32_t w0 = zr_lds_u32(al);
        for (; i + 8 <= n; i += 8) {
            uint32_t w1 = zr_lds_u32(al + i + 4);
            uint32_t w2 = zr_lds_u32(al + i + 8);
            uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32);
            uint64_t v = sh ? (lo >> sh) | ((uint64_t)w2 << (64 - sh)) : lo;
            __builtin_memcpy(dst + i, &v, 8);
            w0 = w2;
        }
    }
    for (; i < n; i++) dst[i] = src4[so + i];
}

__device__ inline int zr_decode_frame_a4(const uint8_t *src, int slen,
                                         uint8_t *dst, int dcap,
                                         const zr_dcell *llt,
                                         const zr_dcell *mlt,
                                         const zr_dcell *oft)
{
    int ip = 0;
    if (slen < 7) return -1;
    if (!(src[0] == 0x28 && src[1] == 0xB5 && src[2] == 0x2F && src[3] == 0xFD))
        return -1;
    ip = 4;
    const uint8_t fhd = src[ip++];
    if (!(fhd == 0x20 || fhd == 0x60 || fhd == 0xA0)) return -1;
    int content;
    if (fhd == 0x20) {
        content = src[ip++];
    } else if (fhd == 0x60) {
        content = 256 + src[ip] + (src[ip + 1] << 8);
        ip += 2;
    } else {
        uint32_t f = 0;
        for (int i = 0; i < 4; i++) f |= (uint32_t)src[ip + i] << (8 * i);
        if (f > (1u << 23)) return -1;
        content = (int)f;
        ip += 4;
    }
    if (content > dcap) return -1;
    const uint32_t bh = (uint32_t)src[ip] | ((uint32_t)src[ip + 1] << 8) |
                        ((uint32_t)src[ip + 2] << 16);
    ip += 3;
    const int btype = (int)((bh >> 1) & 3);
    const int bsize = (int)(bh >> 3);
    if (ip + bsize > slen) return -1;
    if (btype == 0) {                     /* raw block */
        if (bsize != content) return -1;
        zr_lds_copy(dst, src, (uint32_t)ip, (uint32_t)content);
        return content;
    }
    if (btype != 2) return -1;
    const int bend = ip + bsize;

    const uint8_t lh = src[ip];           /* literals: RAW only */
    if ((lh & 3) != 0) return -1;
    int lit_size;
    if (!(lh & 0x04)) { lit_size = lh >> 3; ip += 1; }
    else if (!(lh & 0x08)) { lit_size = (lh >> 4) | ((int)src[ip + 1] << 4); ip += 2; }
    else { lit_size = (lh >> 4) | ((int)src[ip + 1] << 4) | ((int)src[ip + 2] << 12); ip += 3; }
    const uint32_t lit_off = (uint32_t)ip;
    ip += lit_size;
    if (ip > bend) return -1;

    int nseq = src[ip++];
    if (nseq >= 128) {
        if (nseq == 255) { nseq = src[ip] + (src[ip + 1] << 8) + 0x7F00; ip += 2; }
        else { nseq = ((nseq - 128) << 8) + src[ip]; ip += 1; }
    }
    int op = 0, lp = 0;
    if (nseq == 0) {
        if (lit_size != content) return -1;
        zr_lds_copy(dst, src, lit_off, (uint32_t)content);
        return content;
    }
    if (src[ip++] != 0x00) return -1;

    zr_brd br;
    if (zr_brd_init(&br, src + ip, bend - ip) < 0) return -1;
    uint32_t sll = zr_brd_read(&br, ZR_LL_ACCLOG);
    uint32_t sof = zr_brd_read(&br, ZR_OF_ACCLOG);
    uint32_t sml = zr_brd_read(&br, ZR_ML_ACCLOG);

    for (int n = 0; n < nseq; n++) {
        const uint32_t cll = zr_cell_d(llt, sll);
        const uint32_t cml = zr_cell_d(mlt, sml);
        const uint32_t cof = zr_cell_d(oft, sof);
        const uint32_t of_sym = cof & 0xFF, ml_sym = cml & 0xFF, ll_sym = cll & 0xFF;
        const uint32_t of_val = (1u << of_sym) + zr_brd_read(&br, (int)of_sym);
        uint32_t ml = ZR_ML_BASE[ml_sym] + zr_brd_read(&br, ZR_ML_BITS[ml_sym]);
        uint32_t ll = ZR_LL_BASE[ll_sym] + zr_brd_read(&br, ZR_LL_BITS[ll_sym]);
        if (n + 1 < nseq) {
            sll = (cll >> 16) + zr_brd_read(&br, (int)((cll >> 8) & 0xFF));
            sml = (cml >> 16) + zr_brd_read(&br, (int)((cml >> 8) & 0xFF));
            sof = (cof >> 16) + zr_brd_read(&br, (int)((cof >> 8) & 0xFF));
        }
        if (of_val <= 3) return -1;
        const uint32_t off = of_val - 3;
        if (lp + (int)ll > lit_size || op + (int)(ll + ml) > content) return -1;
        zr_lds_copy(dst + op, src, lit_off + (uint32_t)lp, ll);
        op += (int)ll; lp += (int)ll;
        if (off > (uint32_t)op) return -1;
        {   /* match: global->global, unaligned 8B memcpys are fine there */
            uint32_t i = 0;
            if (off >= 8) {
                for (; i + 8 <= ml; i += 8) {
                    uint64_t v;
                    __builtin_memcpy(&v, dst + op + (int)i - (int)off, 8);
                    __builtin_memcpy(dst + op + (int)i, &v, 8);
                }
            }
            for (; i < ml; i++) dst[op + (int)i] = dst[op + (int)i - (int)off];
            op += (int)ml;
        }
    }
    const int rem = lit_size - lp;
    if (op + rem != content) return -1;
    zr_lds_copy(dst + op, src, lit_off + (uint32_t)lp, (uint32_t)rem);
    return content;
}

/* LDS-staged variant: the global kernel's wall is the serial FSE decode's
 * dependent byte loads — each lane walks its own frame, the block's frame
 * working set (~128 x 512 B) blows past L1, so every window refill / literal
 * read is an uncoalesced L2-or-HBM round trip. Here the block first copies
 * its 128 frames into LDS with coalesced dword loads (and the 640 B spec
 * FSE tables once), then each lane decodes ITS frame entirely out of LDS
 * via the aligned-dword decoder above; only the decoded output goes to
 * global. Chosen by launch_decode when the largest frame fits the LDS
 * budget (writer default 512 B zstd segments -> ~72 KB/block, 2 blocks/CU). */
#define ZR_LDS_BLOCK 128
__global__ __launch_bounds__(ZR_LDS_BLOCK) void zr_decode_lds_kernel(
    const uint8_t *__restrict__ data, uint8_t *__restrict__ scratch,
    const SegDesc *__restrict__ segs, uint32_t n, uint32_t stride,
    const zr_dtables *__restrict__ dt, int *__restrict__ err)
{
    extern __shared__ uint8_t zbuf[];   /* [ZR_LDS_BLOCK*stride] | tables */
    zr_dcell *tll = (zr_dcell *)(zbuf + (size_t)ZR_LDS_BLOCK * stride);
    zr_dcell *tml = tll + (1 << ZR_LL_ACCLOG);
    zr_dcell *tof = tml + (1 << ZR_ML_ACCLOG);
    __shared__ uint64_t s_src[ZR_LDS_BLOCK];
    __shared__ uint32_t s_len[ZR_LDS_BLOCK];
    {   /* spec tables: 640 B of 4 B cells, cooperative copy */
        const uint32_t *ts = (const uint32_t *)dt;
        uint32_t *td = (uint32_t *)tll;
        for (uint32_t j = threadIdx.x; j < sizeof(zr_dtables) / 4; j += ZR_LDS_BLOCK)
            td[j] = ts[j];
    }
    const uint32_t base_i = blockIdx.x * ZR_LDS_BLOCK;
    const uint32_t i = base_i + threadIdx.x;
    if (i < n) { s_src[threadIdx.x] = segs[i].src_off; s_len[threadIdx.x] = segs[i].comp_len; }
    else s_len[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t nf = n - base_i < ZR_LDS_BLOCK ? n - base_i : ZR_LDS_BLOCK;
    for (uint32_t f = 0; f < nf; f++) {
        /* coalesced staging: unaligned global dword loads (hardware-
         * tolerated), aligned LDS dword writes */
        const uint8_t *src = data + s_src[f];
        uint32_t *d4 = (uint32_t *)(zbuf + (size_t)f * stride);
        const uint32_t nw = (s_len[f] + 3) >> 2;
        for (uint32_t j = threadIdx.x; j < nw; j += ZR_LDS_BLOCK) {
            uint32_t v;
            __builtin_memcpy(&v, src + 4 * j, 4);
            d4[j] = v;
        }
    }
    __syncthreads();
    if (i >= n) return;
    const SegDesc s = segs[i];
    const int r = zr_decode_frame_a4(zbuf + (size_t)threadIdx.x * stride, (int)s.comp_len,
                                     scratch + s.dst_off, (int)s.decomp_len,
                                     tll, tml, tof);
    if (r != (int)s.decomp_len) atomicOr(err, 32);
}

/* LDS-in + LDS-out variant: PMC on the kernel above shows 86% of wave
 * cycles parked on s_waitcnt — with the frames LDS-resident, the residual
 * latency chain is the OUTPUT path: every match copy is a load-after-store
 * round trip through global L2 (stores bypass L1 on CDNA), serialized by
 * vmcnt waits 8 bytes at a time. Here each lane decodes into its own LDS
 * output slot, so match copies stay in LDS, and the block flushes decoded
 * slots to global with coalesced 16 B stores at the end. Costs ~2x the LDS
 * (1 block/CU at the 512 B writer default) but removes the global round
 * trips from the serial chain. */
__global__ __launch_bounds__(ZR_LDS_BLOCK) void zr_decode_lds2_kernel(
    const uint8_t *__restrict__ data, uint8_t *__restrict__ scratch,
    const SegDesc *__restrict__ segs, uint32_t n, uint32_t stride,
    uint32_t ostride, const zr_dtables *__restrict__ dt, int *__restrict__ err)
{
    extern __shared__ uint8_t zbuf[];   /* [in frames][out slots][tables] */
    uint8_t *obuf = zbuf + (size_t)ZR_LDS_BLOCK * stride;
    zr_dcell *tll = (zr_dcell *)(obuf + (size_t)ZR_LDS_BLOCK * ostride);
    zr_dcell *tml = tll + (1 << ZR_LL_ACCLOG);
    zr_dcell *tof = tml + (1 << ZR_ML_ACCLOG);
    __shared__ uint64_t s_src[ZR_LDS_BLOCK];
    __shared__ uint64_t s_dst[ZR_LDS_BLOCK];
    __shared__ uint32_t s_len[ZR_LDS_BLOCK];
    __shared__ uint32_t s_dlen[ZR_LDS_BLOCK];
    {
        const uint32_t *ts = (const uint32_t *)dt;
        uint32_t *td = (uint32_t *)tll;
        for (uint32_t j = threadIdx.x; j < sizeof(zr_dtables) / 4; j += ZR_LDS_BLOCK)
            td[j] = ts[j];
    }
    const uint32_t base_i = blockIdx.x * ZR_LDS_BLOCK;
    const uint32_t i = base_i + threadIdx.x;
    if (i < n) {
        const SegDesc s = segs[i];
        s_src[threadIdx.x] = s.src_off;
        s_dst[threadIdx.x] = s.dst_off;
        s_len[threadIdx.x] = s.comp_len;
        s_dlen[threadIdx.x] = s.decomp_len;
    } else { s_len[threadIdx.x] = 0; s_dlen[threadIdx.x] = 0; }
    __syncthreads();
    const uint32_t nf = n - base_i < ZR_LDS_BLOCK ? n - base_i : ZR_LDS_BLOCK;
    for (uint32_t f = 0; f < nf; f++) {
        const uint8_t *src = data + s_src[f];
        uint32_t *d4 = (uint32_t *)(zbuf + (size_t)f * stride);
        const uint32_t nw = (s_len[f] + 3) >> 2;
        for (uint32_t j = threadIdx.x; j < nw; j += ZR_LDS_BLOCK) {
            uint32_t v;
            __builtin_memcpy(&v, src + 4 * j, 4);
            d4[j] = v;
        }
    }
    __syncthreads();
    if (i < n) {
        const int r = zr_decode_frame_a4(zbuf + (size_t)threadIdx.x * stride,
                                         (int)s_len[threadIdx.x],
                                         obuf + (size_t)threadIdx.x * ostride,
                                         (int)s_dlen[threadIdx.x],
                                         tll, tml, tof);
        if (r != (int)s_dlen[threadIdx.x]) atomicOr(err, 32);
    }
    __syncthreads();
    for (uint32_t f = 0; f < nf; f++) {     /* coalesced flush, exact dlen */
        uint8_t *dst = scratch + s_dst[f];
        const uint8_t *out = obuf + (size_t)f * ostride;   /* 4-aligned slot */
        const uint32_t dlen = s_dlen[f];
        const uint32_t vec = dlen >> 2;
        for (uint32_t j = threadIdx.x; j < vec; j += ZR_LDS_BLOCK) {
            const uint32_t v = zr_lds_u32(out + 4 * j);
            __builtin_memcpy(dst + 4 * j, &v, 4);   /* global: unaligned ok */
        }
        for (uint32_t j = (vec << 2) + threadIdx.x; j < dlen; j += ZR_LDS_BLOCK)
            dst[j] = out[j];
    }
}

/* =====================================================================
 * device chunk-group pruning (SelectedChunkMask on GPU — SURVEY §8f3)
 * One thread per chunk group evaluates the same CNF refutation as the
 * host loop in cstripe_scan_begin (reference: SelectedChunkMask,
 * columnar_reader.c:1132-1187; OR recursion columnar_customscan.c:770-829),
 * including PG float ordering and the all-NULL-chunk rule. The host only
 * GATHERS the skip entries (a copy pass, no comparisons); every compare
 * runs on device.
 * ===================================================================== */

struct PruneMM { int64_t mn, mx; uint64_t has; };

struct PrunePred {
    int64_t ival;
    double fval;
    uint8_t op, is_float, slot, gend;
};

struct PruneParams {
    uint32_t n_preds;
    PrunePred preds[CSTRIPE_MAX_PREDS];
};

__global__ void chunk_prune_kernel(const PruneMM *__restrict__ mm,
                                   uint32_t n_chunks,
                                   uint8_t *__restrict__ selected,
                                   const PruneParams pp)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    bool sel = true;
    bool group_refuted = true;
    for (uint32_t i = 0; i < pp.n_preds; i++) {
        const PrunePred &p = pp.preds[i];
        const PruneMM e = mm[(size_t)p.slot * n_chunks + c];
        bool ref = false;
        if (e.has) {          /* all-NULL chunks are never refuted */
            if (p.is_float) {
                double mn, mx;
                __builtin_memcpy(&mn, &e.mn, 8);
                __builtin_memcpy(&mx, &e.mx, 8);
                const double cv = p.fval;
                switch (p.op) {     /* PG float ordering (NaN high) */
                    case CSTRIPE_PRED_LT: ref = f64cmp_pg(mn, cv) >= 0; break;
                    case CSTRIPE_PRED_LE: ref = f64cmp_pg(mn, cv) > 0; break;
                    case CSTRIPE_PRED_GT: ref = f64cmp_pg(mx, cv) <= 0; break;
                    case CSTRIPE_PRED_GE: ref = f64cmp_pg(mx, cv) < 0; break;
                    case CSTRIPE_PRED_EQ: ref = f64cmp_pg(cv, mn) < 0 ||
                                                f64cmp_pg(cv, mx) > 0; break;
                    default:              ref = f64cmp_pg(mn, cv) == 0 &&
                                                f64cmp_pg(mx, cv) == 0; break;
                }
            } else {
                const int64_t cv = p.ival;
                switch (p.op) {
                    case CSTRIPE_PRED_LT: ref = e.mn >= cv; break;
                    case CSTRIPE_PRED_LE: ref = e.mn > cv; break;
                    case CSTRIPE_PRED_GT: ref = e.mx <= cv; break;
                    case CSTRIPE_PRED_GE: ref = e.mx < cv; break;
                    case CSTRIPE_PRED_EQ: ref = cv < e.mn || cv > e.mx; break;
                    default:              ref = e.mn == cv && e.mx == cv; break;
                }
            }
        }
        group_refuted &= ref;
        if (p.gend) {
            if (group_refuted) { sel = false; break; }
            group_refuted = true;
        }
    }
    selected[c] = sel ? 1 : 0;
}

int csgpu_prune(cstripe_reader *r, const std::vector<cstripe_pred> &preds,
                std::vector<uint8_t> &selected)
{
    if (!cstripe_gpu_available()) return CSTRIPE_ERR_NOGPU;
    if (preds.empty() || preds.size() > CSTRIPE_MAX_PREDS) return CSTRIPE_ERR_ARG;

    /* distinct predicate columns -> slots */
    PruneParams pp{};
    pp.n_preds = (uint32_t)preds.size();
    uint32_t slot_col[CSTRIPE_MAX_PREDS];
    uint32_t n_slots = 0;
    for (uint32_t i = 0; i < pp.n_preds; i++) {
        const cstripe_pred &p = preds[i];
        uint32_t sl = n_slots;
        for (uint32_t j = 0; j < n_slots; j++)
            if (slot_col[j] == p.column) { sl = j; break; }
        if (sl == n_slots) slot_col[n_slots++] = p.column;
        const uint8_t ty = r->cols[p.column].type;
        pp.preds[i].ival = p.ival;
        pp.preds[i].fval = p.fval;
        pp.preds[i].op = p.op;
        pp.preds[i].is_float = ty == CSTRIPE_F32 || ty == CSTRIPE_F64;
        pp.preds[i].slot = (uint8_t)sl;
        pp.preds[i].gend = i + 1 == pp.n_preds ||
                           preds[i + 1].or_group != preds[i].or_group;
    }

    uint64_t n_chunks = 0;
    for (const auto &st : r->stripes) n_chunks += st.meta.chunk_count;
    if (n_chunks == 0) { selected.clear(); return CSTRIPE_OK; }

    /* gather skip entries per slot, global chunk order */
    std::vector<PruneMM> h_mm((size_t)n_slots * n_chunks);
    uint64_t ci = 0;
    for (const auto &st : r->stripes) {
        for (uint32_t k = 0; k < st.meta.chunk_count; k++, ci++) {
            for (uint32_t sl = 0; sl < n_slots; sl++) {
                const csf_skipnode &nd = st.nodes[slot_col[sl]][k].n;
                PruneMM &e = h_mm[(size_t)sl * n_chunks + ci];
                e.mn = nd.min_i;
                e.mx = nd.max_i;
                e.has = nd.has_min_max;
            }
        }
    }

    PruneMM *d_mm = nullptr;
    uint8_t *d_sel = nullptr;
    #define PR_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) { \
        cs_set_err("prune: %s", hipGetErrorString(_e)); \
        if (d_mm) (void)hipFree(d_mm); if (d_sel) (void)hipFree(d_sel); \
        return CSTRIPE_ERR; } } while (0)
    PR_TRY(hipMalloc(&d_mm, h_mm.size() * sizeof(PruneMM)));
    PR_TRY(hipMalloc(&d_sel, n_chunks));
    PR_TRY(hipMemcpy(d_mm, h_mm.data(), h_mm.size() * sizeof(PruneMM),
                     hipMemcpyHostToDevice));
    const uint32_t grid = (uint32_t)((n_chunks + 255) / 256);
    hipLaunchKernelGGL(chunk_prune_kernel, dim3(grid), dim3(256), 0, 0,
                       d_mm, (uint32_t)n_chunks, d_sel, pp);
    PR_TRY(hipGetLastError());
    selected.resize(n_chunks);
    PR_TRY(hipMemcpy(selected.data(), d_sel, n_chunks, hipMemcpyDeviceToHost));
    #undef PR_TRY
    (void)hipFree(d_mm);
    (void)hipFree(d_sel);
    return CSTRIPE_OK;
}

/* =====================================================================
 * staging
 * ===================================================================== */

static uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

/* single-segment chunk with a CLOSED-FORM canonical stream (lz4 P/CONST/LIT
 * or restricted-zstd P/CONST, format.h): staged compressed, read in place */
static inline bool cs_node_canon(const cs_skipnode &nd)
{
    if (nd.n.n_segs != 1) return false;
    const uint8_t m = nd.seg_modes[0];
    if (nd.n.comp_type == CSTRIPE_COMP_LZ4)
        return m != CSF_SEGMODE_GENERIC;
    if (nd.n.comp_type == CSTRIPE_COMP_ZSTD)
        return m == CSF_SEGMODE_ZR_CONST ||
               (m > CSF_SEGMODE_ZRP_BASE && m <= CSF_SEGMODE_ZRP_BASE + 4) ||
               (m >= CSF_SEGMODE_ZR4B_BASE && m <= CSF_SEGMODE_ZR4_CONST);
    return false;
}

void csgpu_release(cstripe_scan *s)
{
    if (!s || !s->gpu) return;
    cs_gpu_state *g = s->gpu;
    #define HIP_DROP(x) do { hipError_t _e = (x); (void)_e; } while (0)
    if (g->d_data) HIP_DROP(hipFree(g->d_data));
    if (g->d_scratch) HIP_DROP(hipFree(g->d_scratch));
    if (g->d_rank) HIP_DROP(hipFree(g->d_rank));
    if (g->d_segs) HIP_DROP(hipFree(g->d_segs));
    if (g->d_groups) HIP_DROP(hipFree(g->d_groups));
    if (g->d_colloc) HIP_DROP(hipFree(g->d_colloc));
    if (g->d_block) HIP_DROP(hipFree(g->d_block));
    if (g->d_final) HIP_DROP(hipFree(g->d_final));
    if (g->d_final2) HIP_DROP(hipFree(g->d_final2));
    if (g->d_gkeys) HIP_DROP(hipFree(g->d_gkeys));
    if (g->d_gcells) HIP_DROP(hipFree(g->d_gcells));
    if (g->d_gfkeys) HIP_DROP(hipFree(g->d_gfkeys));
    if (g->d_gfcells) HIP_DROP(hipFree(g->d_gfcells));
    if (g->d_gn) HIP_DROP(hipFree(g->d_gn));
    if (g->d_tmp) HIP_DROP(hipFree(g->d_tmp));
    if (g->d_zsegs) HIP_DROP(hipFree(g->d_zsegs));
    if (g->d_zrtab) HIP_DROP(hipFree(g->d_zrtab));
    if (g->d_tiles) HIP_DROP(hipFree(g->d_tiles));
    if (g->d_error) HIP_DROP(hipFree(g->d_error));
    if (g->d_sel_mask) HIP_DROP(hipFree(g->d_sel_mask));
    if (g->d_sel_counts) HIP_DROP(hipFree(g->d_sel_counts));
    if (g->d_sel_bases) HIP_DROP(hipFree(g->d_sel_bases));
    if (g->d_sel_total) HIP_DROP(hipFree(g->d_sel_total));
    if (g->d_sel_rowbase) HIP_DROP(hipFree(g->d_sel_rowbase));
    if (g->d_sel_out) HIP_DROP(hipFree(g->d_sel_out));
    if (g->d_hkeys) HIP_DROP(hipFree(g->d_hkeys));
    if (g->d_hcells) HIP_DROP(hipFree(g->d_hcells));
    if (g->d_hokeys) HIP_DROP(hipFree(g->d_hokeys));
    if (g->d_hocells) HIP_DROP(hipFree(g->d_hocells));
    if (g->d_hcount) HIP_DROP(hipFree(g->d_hcount));
    if (g->d_tn_keys) HIP_DROP(hipFree(g->d_tn_keys));
    if (g->d_tn_okeys) HIP_DROP(hipFree(g->d_tn_okeys));
    if (g->d_tn_state) HIP_DROP(hipFree(g->d_tn_state));
    if (g->d_tn_mask) HIP_DROP(hipFree(g->d_tn_mask));
    if (g->d_tn_eq) HIP_DROP(hipFree(g->d_tn_eq));
    if (g->d_tn_counts) HIP_DROP(hipFree(g->d_tn_counts));
    if (g->d_tn_tbases) HIP_DROP(hipFree(g->d_tn_tbases));
    if (g->d_tn_bases) HIP_DROP(hipFree(g->d_tn_bases));
    if (g->d_tn_total) HIP_DROP(hipFree(g->d_tn_total));
    if (g->d_tn_emit) HIP_DROP(hipFree(g->d_tn_emit));
    if (g->d_tn_out) HIP_DROP(hipFree(g->d_tn_out));
    if (g->d_tn_perm) HIP_DROP(hipFree(g->d_tn_perm));
    if (g->d_gt_kept) HIP_DROP(hipFree(g->d_gt_kept));
    if (g->d_gt_ord) HIP_DROP(hipFree(g->d_gt_ord));
    if (g->d_gt_tie) HIP_DROP(hipFree(g->d_gt_tie));
    if (g->d_gt_state) HIP_DROP(hipFree(g->d_gt_state));
    if (g->d_gt_sel) HIP_DROP(hipFree(g->d_gt_sel));
    if (g->d_gt_out) HIP_DROP(hipFree(g->d_gt_out));
    for (void *b : g->set_bufs) if (b) HIP_DROP(hipFree(b));
    for (hipEvent_t e : g->gev) if (e) HIP_DROP(hipEventDestroy(e));
    for (hipEvent_t e : g->tev) if (e) HIP_DROP(hipEventDestroy(e));
    for (hipEvent_t e : g->hev) if (e) HIP_DROP(hipEventDestroy(e));
    for (hipEvent_t e : g->sev) if (e) HIP_DROP(hipEventDestroy(e));
    if (g->ev0) HIP_DROP(hipEventDestroy(g->ev0));
    if (g->ev1) HIP_DROP(hipEventDestroy(g->ev1));
    if (g->ev2) HIP_DROP(hipEventDestroy(g->ev2));
    if (g->stream) HIP_DROP(hipStreamDestroy(g->stream));
    #undef HIP_DROP
    delete g;
    s->gpu = nullptr;
    for (cs_value_set &vs : s->sets) { vs.form = 0; vs.form_size = 0; }
    for (cs_lookup &lk : s->lookups) { lk.form = 0; lk.form_size = 0; }
    for (cs_expr &ex : s->exprs) { ex.lo = ex.hi = 0; ex.n_present = 0; }
}

uint64_t csgpu_staged_bytes(const cstripe_scan *s)
{
    return s->gpu ? s->gpu->data_bytes : 0;
}

/* temporary device buffers and events of one VARTEXT dictionary build
 * (vartext_build, below launch_decode); freed when the stage call returns */
struct VtTemps {
    void *bufs[16] = {nullptr};
    uint32_t n_bufs = 0;
    hipEvent_t ev[8] = {nullptr};
    template <typename T>
    hipError_t alloc(T *&p, uint64_t bytes)
    {
        if (n_bufs >= sizeof(bufs) / sizeof(bufs[0])) return hipErrorOutOfMemory;   /* bufs[] full */
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
        if (e == hipSuccess) { bufs[n_bufs++] = q; p = (T *)q; }
        return e;
    }
    /* per-column buffers go back early; the rest at release() */
    void free_from(uint32_t first)
    {
        while (n_bufs > first) { hipError_t e = hipFree(bufs[--n_bufs]); (void)e; }
    }
    void release()
    {
        free_from(0);
        for (hipEvent_t &e : ev)
            if (e) { hipError_t r = hipEventDestroy(e); (void)r; e = nullptr; }
    }
};
static int vartext_build(cstripe_scan *s, VtTemps &vt);
static int sets_build(cstripe_scan *s, VtTemps &st);
static int lookups_build(cstripe_scan *s, VtTemps &lt);
static int exprs_build(cstripe_scan *s, VtTemps &et);

int csgpu_stage(cstripe_scan *s, int device_id)
{
    if (!cstripe_gpu_available()) { cs_set_err("no HIP device visible — the cstripe GPU path requires an MI355X (no CPU fallback)"); return CSTRIPE_ERR_NOGPU; }
    if (s->gpu) csgpu_release(s);
    s->text_dicts.clear();

    cstripe_reader *r = s->r;
    auto *g = new cs_gpu_state();
    s->gpu = g;
    if (device_id >= 0) {
        if (hipSetDevice(device_id) != hipSuccess) { cs_set_err("hipSetDevice(%d) failed", device_id); csgpu_release(s); return CSTRIPE_ERR; }
        g->device = device_id;
    } else {
        (void)hipGetDevice(&g->device);
    }

    /* projected column slots */
    for (int i = 0; i < 64; i++) g->proj_of_col[i] = -1;
    uint32_t n_proj = 0;
    for (uint32_t c = 0; c < r->head.column_count; c++) {
        if (s->cols_mask & (1ull << c)) {
            if (n_proj >= MAX_PROJ) { cs_set_err("too many projected columns"); csgpu_release(s); return CSTRIPE_ERR_ARG; }
            g->proj_of_col[c] = (int)n_proj;
            g->proj_type[n_proj] = r->cols[c].type;
            n_proj++;
        }
    }
    if (n_proj == 0) { cs_set_err("empty projection"); csgpu_release(s); return CSTRIPE_ERR_ARG; }
    /* member slots of the IN / NOT IN predicates, after the table columns */
    const uint32_t n_tab = n_proj;
    g->mpred_slot.assign(s->preds.size(), -1);
    for (size_t i = 0; i < s->preds.size(); i++) {
        const cstripe_pred &q = s->preds[i];
        const bool like = cs_pred_is_like(q);
        if (q.op != CSTRIPE_PRED_IN && q.op != CSTRIPE_PRED_NOT_IN && !like) continue;
        int found = -1;
        for (size_t m = 0; m < g->mslots.size(); m++) {
            const auto &ms = g->mslots[m];
            if (ms.col != q.column || ms.like != like) continue;
            if (like ? s->text_consts[ms.set] == s->text_consts[(size_t)q.ival]
                     : ms.set == (uint32_t)q.ival) found = (int)m;
        }
        if (found < 0) {
            if (n_proj >= MAX_PROJ) {
                cs_set_err("gpu_stage: %u projected columns plus the membership columns of the "
                           "IN / NOT IN and LIKE / NOT LIKE predicates exceed the %d slots of one "
                           "scan", n_tab, MAX_PROJ);
                csgpu_release(s);
                return CSTRIPE_ERR_ARG;
            }
            found = (int)g->mslots.size();
            g->mslots.push_back({q.column, (uint32_t)q.ival, n_proj, like});
            g->proj_type[n_proj] = CSTRIPE_I8;
            n_proj++;
        }
        g->mpred_slot[i] = found;
    }
    if (!g->mslots.empty()) g->fusable = false;
    /* read form of the pattern-matched columns: STREAM when nothing reads the
     * column's values (need_mask), DICT otherwise; CSTRIPE_LIKE_FORM=dict
     * forces DICT, =stream changes nothing (a column that needs ranks keeps
     * them) */
    g->like_form.assign(r->head.column_count, CSTRIPE_LIKE_FORM_NONE);
    {
        const char *lf = getenv("CSTRIPE_LIKE_FORM");
        const bool force_dict = lf && !strcmp(lf, "dict");
        for (const auto &ms : g->mslots)
            if (ms.like)
                g->like_form[ms.col] = (uint8_t)(
                    (s->need_mask & (1ull << ms.col)) || force_dict ? CSTRIPE_LIKE_FORM_DICT
                                                                    : CSTRIPE_LIKE_FORM_STREAM);
    }
    s->like_forms = g->like_form;
    s->last_like_match_ms = s->last_like_apply_ms = 0;
    /* derived slots of the lookups' payload columns, after the member slots */
    for (size_t l = 0; l < s->lookups.size(); l++)
        for (uint32_t pl = 0; pl < s->lookups[l].n_payloads; pl++) {
            if (n_proj >= MAX_PROJ) {
                cs_set_err("gpu_stage: %u projected columns plus the derived columns of the "
                           "lookups exceed the %d slots of one scan (lookup %u)",
                           n_proj, MAX_PROJ, (unsigned)l);
                csgpu_release(s);
                return CSTRIPE_ERR_ARG;
            }
            g->dslots.push_back({(uint32_t)l, pl, n_proj});
            g->proj_of_col[s->lookups[l].first_col + pl] = (int)n_proj;
            g->proj_type[n_proj] = CSTRIPE_I64;
            n_proj++;
        }
    if (!g->dslots.empty()) { g->fusable = false; g->all_dense = false; }
    /* computed slots of the expressions, after the derived slots */
    for (size_t e = 0; e < s->exprs.size(); e++) {
        if (n_proj >= MAX_PROJ) {
            cs_set_err("gpu_stage: %u projected columns plus the computed columns of the "
                       "expressions exceed the %d slots of one scan (expression %u)",
                       n_proj, MAX_PROJ, (unsigned)e);
            csgpu_release(s);
            return CSTRIPE_ERR_ARG;
        }
        g->eslots.push_back(n_proj);
        g->proj_of_col[s->exprs[e].first_col] = (int)n_proj;
        g->proj_type[n_proj] = CSTRIPE_I64;
        n_proj++;
    }
    if (!g->eslots.empty()) { g->fusable = false; g->all_dense = false; }
    g->n_proj = n_proj;
    g->n_groups = (uint32_t)s->sel.size();

    /* host pass 1: compute layout sizes */
    uint64_t data_bytes = 0, scratch_bytes = 0, rank_words = 0;
    uint32_t n_segs = 0, n_zsegs = 0;
    bool zstd_host = false;
    bool any_vartext = false;
    for (uint32_t c = 0; c < r->head.column_count; c++)
        any_vartext |= g->proj_of_col[c] >= 0 && r->cols[c].type == CSTRIPE_VARTEXT;
    for (const auto &sc : s->sel) {
        const cs_stripe_info &st = r->stripes[sc.stripe];
        uint32_t rows = st.group_rows[sc.chunk];
        for (uint32_t c = 0; c < r->head.column_count; c++) {
            if (g->proj_of_col[c] < 0) continue;
            const cs_skipnode &nd = st.nodes[c][sc.chunk];
            data_bytes = align_up(data_bytes, 8) + align_up((rows + 7) / 8, 8); /* exists, 8B padded */
            if (r->cols[c].type == CSTRIPE_VARTEXT) {
                /* read as int32 dictionary ranks: n_present entries in a
                 * scratch region no decode segment writes (vartext_build);
                 * the byte stream itself is staged to temporary buffers. A
                 * STREAM-form column is only pattern-matched: no ranks */
                if (g->like_form[c] != CSTRIPE_LIKE_FORM_STREAM)
                    scratch_bytes = align_up(scratch_bytes, 16) + align_up((uint64_t)nd.n.n_present * 4, 16);
                any_vartext = true;
                if (nd.n.n_present != nd.n.row_count)
                    rank_words += (rows + 63) / 64;
                continue;
            }
            const bool canon = cs_node_canon(nd);
            bool zr_dev = !canon && nd.n.comp_type == CSTRIPE_COMP_ZSTD;
            if (zr_dev)
                for (uint8_t m : nd.seg_modes)
                    if (m != CSF_SEGMODE_ZR) { zr_dev = false; break; }
            if (canon) {
                /* canonical stream: values are read closed-form from the
                 * compressed bytes — no scratch, no decode segments */
                data_bytes = align_up(data_bytes, 16) + align_up(nd.n.value_len, 16);
            } else if (zr_dev) {
                /* restricted-zstd frames: staged compressed, decoded on
                 * device into scratch (zr_decode_kernel) */
                data_bytes = align_up(data_bytes, 16) + align_up(nd.n.value_len, 16);
                scratch_bytes = align_up(scratch_bytes, 16) + align_up(nd.n.decompressed_size, 16);
                n_zsegs += nd.n.n_segs;
            } else if (nd.n.comp_type == CSTRIPE_COMP_LZ4) {
                data_bytes = align_up(data_bytes, 16) + align_up(nd.n.value_len, 16);
                scratch_bytes = align_up(scratch_bytes, 16) + align_up(nd.n.decompressed_size, 16);
                n_segs += nd.n.n_segs;
            } else { /* NONE staged raw; ZSTD host-decoded at stage (documented fallback) */
                if (nd.n.comp_type == CSTRIPE_COMP_ZSTD || nd.n.comp_type == CSTRIPE_COMP_PGLZ) zstd_host = true;
                data_bytes = align_up(data_bytes, 16) + align_up(nd.n.decompressed_size, 16);
            }
            if (nd.n.n_present != nd.n.row_count)
                rank_words += (rows + 63) / 64;
        }
        /* membership bytes: n_present entries in a scratch region no decode
         * segment writes, padded so the probe's dword stores stay inside */
        for (const auto &ms : g->mslots)
            scratch_bytes = align_up(scratch_bytes, 16) +
                            align_up((uint64_t)st.nodes[ms.col][sc.chunk].n.n_present, 16);
        /* derived columns: per lookup one device-written exists bitmap and
         * rank table (the payloads share them), per payload room for one
         * value per non-NULL key, in a scratch region no decode segment
         * writes */
        for (const auto &lk : s->lookups) {
            data_bytes = align_up(data_bytes, 8) + align_up((rows + 7) / 8, 8);
            rank_words += (rows + 63) / 64;
            for (uint32_t pl = 0; pl < lk.n_payloads; pl++)
                scratch_bytes = align_up(scratch_bytes, 16) +
                                align_up((uint64_t)st.nodes[lk.key_column][sc.chunk].n.n_present * 8, 16);
        }
        /* computed columns: per expression a device-written exists bitmap
         * and rank table and room for one value per ROW (the result's NULL
         * count is not known in advance), in a scratch region no decode
         * segment writes */
        for (size_t e = 0; e < g->eslots.size(); e++) {
            data_bytes = align_up(data_bytes, 8) + align_up((rows + 7) / 8, 8);
            rank_words += (rows + 63) / 64;
            scratch_bytes = align_up(scratch_bytes, 16) + align_up((uint64_t)rows * 8, 16);
        }
    }
    (void)zstd_host;
    if (any_vartext || !g->mslots.empty() || !g->dslots.empty() || !g->eslots.empty())
        scratch_bytes += 64;        /* the R-row windowed loads of the dense
                                     * kernels reach up to R-1 entries past a
                                     * rank array's end */

    uint32_t tiles_pg = (r->head.chunk_row_limit + TILE_ROWS - 1) / TILE_ROWS;
    if (tiles_pg == 0) tiles_pg = 1;
    uint64_t n_tiles_max = 0;
    for (const auto &sc : s->sel)
        n_tiles_max += (r->stripes[sc.stripe].group_rows[sc.chunk] + 2047) / 2048;
    uint64_t max_blocks = (uint64_t)g->n_groups * tiles_pg;
    if (n_tiles_max > max_blocks) max_blocks = n_tiles_max;
    g->max_blocks = (uint32_t)max_blocks;

    HIP_TRY(hipStreamCreate(&g->stream));
    HIP_TRY(hipEventCreate(&g->ev0));
    HIP_TRY(hipEventCreate(&g->ev1));
    HIP_TRY(hipEventCreate(&g->ev2));
    data_bytes += 128;              /* window read slack: R-row extraction
                                     * windows reach up to ~60 B past the
                                     * last region's stream end. Sized for
                                     * the R=8 windows of col_multi and
                                     * multi_agg_kernel_ov (ov_load): a larger
                                     * R or a wider window there needs a
                                     * larger slack here */
    if (data_bytes) HIP_TRY(hipMalloc(&g->d_data, data_bytes));
    if (scratch_bytes) HIP_TRY(hipMalloc(&g->d_scratch, scratch_bytes));
    if (rank_words) HIP_TRY(hipMalloc(&g->d_rank, rank_words * 4));
    if (n_segs) HIP_TRY(hipMalloc(&g->d_segs, (uint64_t)n_segs * sizeof(SegDesc)));
    if (n_zsegs) {
        HIP_TRY(hipMalloc(&g->d_zsegs, (uint64_t)n_zsegs * sizeof(SegDesc)));
        HIP_TRY(hipMalloc(&g->d_zrtab, sizeof(zr_dtables)));
    }
    HIP_TRY(hipMalloc(&g->d_groups, (uint64_t)g->n_groups * sizeof(GroupDesc)));
    HIP_TRY(hipMalloc(&g->d_colloc, (uint64_t)g->n_groups * n_proj * sizeof(ColLoc)));
    HIP_TRY(hipMalloc(&g->d_block, max_blocks * MAX_AGGS * sizeof(AccCell)));
    HIP_TRY(hipMalloc(&g->d_final, MAX_AGGS * sizeof(AccCell)));
    HIP_TRY(hipMalloc(&g->d_final2, (uint64_t)240 * MAX_AGGS * sizeof(AccCell)));
    HIP_TRY(hipMalloc(&g->d_error, sizeof(int)));
    g->data_bytes = data_bytes;
    g->scratch_bytes = scratch_bytes;
    g->n_segs = n_segs;
    g->n_zsegs = n_zsegs;

    /* host pass 2: build staging buffer + descriptors */
    std::vector<uint8_t> h_data(data_bytes, 0);
    std::vector<uint32_t> h_rank;
    h_rank.reserve(rank_words);
    std::vector<SegDesc> h_segs;
    h_segs.reserve(n_segs);
    std::vector<SegDesc> h_zsegs;
    h_zsegs.reserve(n_zsegs);
    std::vector<uint32_t> seg_start((uint64_t)g->n_groups * n_proj, 0);
    g->col_scratch.assign(n_proj, 0);
    if (n_proj > 4) g->fusable = false;
    std::vector<GroupDesc> h_groups(g->n_groups);
    std::vector<ColLoc> h_colloc((uint64_t)g->n_groups * n_proj);
    g->scratch_off.assign((uint64_t)g->n_groups * n_proj, ~0ull);

    uint64_t dpos = 0, spos = 0;
    std::vector<uint8_t> tmp;   /* zstd host-decode scratch */
    for (uint32_t gi = 0; gi < g->n_groups; gi++) {
        const cs_selchunk &sc = s->sel[gi];
        const cs_stripe_info &st = r->stripes[sc.stripe];
        uint32_t rows = st.group_rows[sc.chunk];
        h_groups[gi].row_count = rows;
        h_groups[gi].colbase = gi * n_proj;
        const uint8_t *stripe_base = r->stripe_base(st);
        for (uint32_t c = 0; c < r->head.column_count; c++) {
            int pj = g->proj_of_col[c];
            if (pj < 0) continue;
            const cs_skipnode &nd = st.nodes[c][sc.chunk];
            ColLoc cl{};
            cl.type = r->cols[c].type;
            cl.width = (uint8_t)csf_type_width(cl.type);
            bool dense = (nd.n.n_present == nd.n.row_count);

            /* exists bitmap (8B padded) */
            dpos = align_up(dpos, 8);
            cl.exists_off = dpos;
            memcpy(h_data.data() + dpos, stripe_base + nd.n.exists_off, nd.n.exists_len);
            dpos += align_up((rows + 7) / 8, 8);

            if (!dense) {
                cl.rank_off = (uint32_t)h_rank.size();
                uint32_t words = (rows + 63) / 64;
                const uint8_t *eb = stripe_base + nd.n.exists_off;
                uint32_t run = 0;
                for (uint32_t w = 0; w < words; w++) {
                    h_rank.push_back(run);
                    uint64_t wv = 0;
                    uint32_t nb = (uint32_t)nd.n.exists_len - w * 8 >= 8 ? 8 : (uint32_t)nd.n.exists_len - w * 8;
                    memcpy(&wv, eb + w * 8, nb);
                    run += (uint32_t)__builtin_popcountll(wv);
                }
            } else {
                cl.flags |= 2;
            }
            if (!(cl.flags & 2)) g->all_dense = false;
            if (r->cols[c].type == CSTRIPE_VARTEXT) {
                /* the column reads as I32 ranks in scratch, dense or sparse
                 * through the rank table above; vartext_build fills the
                 * region after the uploads. Never canonical or fusable, and
                 * launch_decode has nothing to do for it (col_scratch 0). */
                cl.type = CSTRIPE_I32;
                cl.width = 4;
                cl.flags |= 1;
                if (g->like_form[c] != CSTRIPE_LIKE_FORM_STREAM) {
                    spos = align_up(spos, 16);
                    cl.val_off = spos;
                    spos += align_up((uint64_t)nd.n.n_present * 4, 16);
                }   /* else: no rank region; every surface that would read
                     * the column refuses it (like_stream_refused) */
                g->fusable = false;
                h_colloc[(uint64_t)gi * n_proj + pj] = cl;
                continue;
            }
            const bool canon = cs_node_canon(nd);
            if (canon || !(cl.flags & 2) || cl.type != CSTRIPE_I64 ||
                nd.n.comp_type != CSTRIPE_COMP_LZ4)
                g->fusable = false;
            bool zr_dev = !canon && nd.n.comp_type == CSTRIPE_COMP_ZSTD;
            if (zr_dev)
                for (uint8_t m : nd.seg_modes)
                    if (m != CSF_SEGMODE_ZR) { zr_dev = false; break; }
            if (zr_dev) {
                g->col_scratch[pj] = 1;
                dpos = align_up(dpos, 16);
                memcpy(h_data.data() + dpos, stripe_base + nd.n.value_off, nd.n.value_len);
                spos = align_up(spos, 16);
                cl.val_off = spos;
                cl.flags |= 1;                    /* values land in scratch */
                g->scratch_off[(uint64_t)gi * n_proj + pj] = spos;
                for (const csf_seg &sg : st.nodes[c][sc.chunk].segs) {
                    SegDesc sd;
                    sd.src_off = dpos + sg.comp_off;
                    sd.dst_off = spos + sg.decomp_off;
                    sd.comp_len = sg.comp_len;
                    sd.decomp_len = sg.decomp_len;
                    if (sg.comp_len > g->max_zseg_comp) g->max_zseg_comp = sg.comp_len;
                    if (sd.decomp_len > g->max_zseg_dlen) g->max_zseg_dlen = sd.decomp_len;
                    h_zsegs.push_back(sd);
                }
                dpos += align_up(nd.n.value_len, 16);
                spos += align_up(nd.n.decompressed_size, 16);
            } else if (canon) {
                /* stage the compressed stream; kernels read values straight
                 * out of it (col_value canonical path) */
                dpos = align_up(dpos, 16);
                cl.val_off = dpos;
                memcpy(h_data.data() + dpos, stripe_base + nd.n.value_off, nd.n.value_len);
                dpos += align_up(nd.n.value_len, 16);
                cl.flags |= 4;
                cl.mode = nd.seg_modes[0];
                const uint8_t *strm = stripe_base + nd.n.value_off;
                if (cl.mode == CSF_SEGMODE_LIT) {
                    cl.hval = (int64_t)csf_canon_lit_hdr(nd.segs[0].decomp_len);
                } else if ((cl.mode & 0xF8u) == CSF_SEGMODE_ZR4B_BASE) {
                    uint32_t s0;
                    memcpy(&s0, strm + 15, 4);       /* slot0 at lit offset 0 */
                    if (cl.mode == CSF_SEGMODE_ZR4_CONST) {
                        cl.hval = (int64_t)s0;
                    } else {
                        cl.L = (uint8_t)(cl.mode & 0x3);
                        cl.hval = (int64_t)(s0 & ~(0xFFu << (8u * cl.L)));
                    }
                } else {
                    /* v0 full: first literal byte — offset 1 in a canonical
                     * LZ4 block (token first), 15 in a canonical zstd frame
                     * (fixed header, format.h) */
                    const bool zrm = cl.mode >= CSF_SEGMODE_ZRP_BASE;
                    uint64_t v0;
                    memcpy(&v0, strm + (zrm ? 15 : 1), 8);
                    if (cl.mode == CSF_SEGMODE_CONST ||
                        cl.mode == CSF_SEGMODE_ZR_CONST) {
                        cl.hval = (int64_t)v0;
                    } else {                      /* P(L) */
                        cl.L = (uint8_t)(cl.mode & 0xF);
                        const uint64_t m = (~0ull) >> ((8u - cl.L) * 8u);
                        cl.hval = (int64_t)(v0 & ~m);
                    }
                }
            } else if (nd.n.comp_type == CSTRIPE_COMP_LZ4) {
                dpos = align_up(dpos, 16);
                memcpy(h_data.data() + dpos, stripe_base + nd.n.value_off, nd.n.value_len);
                spos = align_up(spos, 16);
                cl.val_off = spos;
                cl.flags |= 1;
                g->scratch_off[(uint64_t)gi * n_proj + pj] = spos;
                seg_start[(uint64_t)gi * n_proj + pj] = (uint32_t)h_segs.size();
                g->col_scratch[pj] = 1;
                uint32_t segi = 0;
                const auto &seglist = st.nodes[c][sc.chunk].segs;
                for (const csf_seg &sg : seglist) {
                    /* non-final segments exactly 256 B, final <= 256 B: the
                     * fused kernel maps row -> lane region as byteoff>>8 and
                     * counts tile segments as ceil(bytes/256), so an absorbed
                     * 257-271 B final segment would read the wrong region
                     * and overrun the segment list (round-1 advisor) */
                    if (sg.decomp_off != segi * 256u ||
                        (segi + 1 < seglist.size() ? sg.decomp_len != 256
                                                   : sg.decomp_len > 256)) {
                        g->fusable = false;
                    }
                    segi++;
                }
                for (const csf_seg &sg : st.nodes[c][sc.chunk].segs) {
                    SegDesc sd;
                    sd.src_off = dpos + sg.comp_off;
                    sd.dst_off = spos + sg.decomp_off;
                    sd.comp_len = sg.comp_len;
                    sd.decomp_len = sg.decomp_len;
                    if (sg.comp_len > g->max_seg_comp) g->max_seg_comp = sg.comp_len;
                    if (sg.decomp_len > g->max_seg_dlen) g->max_seg_dlen = sg.decomp_len;
                    if (sg.decomp_off % 16 != 0) g->segs_16aligned = false;
                    h_segs.push_back(sd);
                }
                dpos += align_up(nd.n.value_len, 16);
                spos += align_up(nd.n.decompressed_size, 16);
            } else if (nd.n.comp_type == CSTRIPE_COMP_NONE) {
                dpos = align_up(dpos, 16);
                cl.val_off = dpos;
                memcpy(h_data.data() + dpos, stripe_base + nd.n.value_off, nd.n.value_len);
                dpos += align_up(nd.n.value_len, 16);
            } else if (nd.n.comp_type == CSTRIPE_COMP_ZSTD ||
                       nd.n.comp_type == CSTRIPE_COMP_PGLZ) {
                /* host-decode at stage (zstd: documented fallback, GPU zstd
                 * is a later item — SURVEY.md §8f(1); pglz is host-only by
                 * design: reference-migrated tables read correctly) */
                dpos = align_up(dpos, 16);
                cl.val_off = dpos;
                tmp.resize(nd.n.decompressed_size);
                for (const csf_seg &sg : st.nodes[c][sc.chunk].segs) {
                    if (nd.n.comp_type == CSTRIPE_COMP_ZSTD) {
                        size_t zr = ZSTD_decompress(tmp.data() + sg.decomp_off, sg.decomp_len,
                                                    stripe_base + nd.n.value_off + sg.comp_off, sg.comp_len);
                        if (ZSTD_isError(zr) || zr != sg.decomp_len) { cs_set_err("zstd host decode failed"); csgpu_release(s); return CSTRIPE_ERR_FORMAT; }
                    } else {
                        const uint8_t *pb = stripe_base + nd.n.value_off + sg.comp_off;
                        if (sg.comp_len < CSPGLZ_HDRSZ ||
                            cspglz_varsize(pb) != sg.comp_len ||
                            cspglz_rawsize(pb) != (int32_t)sg.decomp_len ||
                            cspglz_decompress(pb + CSPGLZ_HDRSZ,
                                              (int32_t)(sg.comp_len - CSPGLZ_HDRSZ),
                                              tmp.data() + sg.decomp_off,
                                              (int32_t)sg.decomp_len) < 0) {
                            cs_set_err("pglz host decode failed");
                            csgpu_release(s);
                            return CSTRIPE_ERR_FORMAT;
                        }
                    }
                }
                memcpy(h_data.data() + dpos, tmp.data(), tmp.size());
                dpos += align_up(nd.n.decompressed_size, 16);
            } else {
                cs_set_err("unsupported chunk compression %d", nd.n.comp_type);
                csgpu_release(s);
                return CSTRIPE_ERR_FORMAT;
            }
            h_colloc[(uint64_t)gi * n_proj + pj] = cl;
        }
        for (const auto &ms : g->mslots) {
            /* the member column reads like the key column — same exists
             * bitmap, rank table and dense flag — with one byte per present
             * value, filled by the probe kernel (sets_build) */
            const ColLoc &key = h_colloc[(uint64_t)gi * n_proj + g->proj_of_col[ms.col]];
            ColLoc cl{};
            cl.type = CSTRIPE_I8;
            cl.width = 1;
            cl.exists_off = key.exists_off;
            cl.rank_off = key.rank_off;
            cl.flags = (uint16_t)((key.flags & 2) | 1);
            spos = align_up(spos, 16);
            cl.val_off = spos;
            spos += align_up((uint64_t)st.nodes[ms.col][sc.chunk].n.n_present, 16);
            h_colloc[(uint64_t)gi * n_proj + ms.proj] = cl;
        }
        for (size_t l = 0, ds = 0; l < s->lookups.size(); l++) {
            /* a derived column reads as a sparse I64 column in scratch; its
             * bitmap (zero here), rank words and values are written on the
             * device (lookups_build) */
            const cs_lookup &lk = s->lookups[l];
            ColLoc cl{};
            cl.type = CSTRIPE_I64;
            cl.width = 8;
            cl.flags = 1;
            dpos = align_up(dpos, 8);
            cl.exists_off = dpos;
            dpos += align_up((rows + 7) / 8, 8);
            cl.rank_off = (uint32_t)h_rank.size();
            h_rank.resize(h_rank.size() + (rows + 63) / 64, 0);
            for (uint32_t pl = 0; pl < lk.n_payloads; pl++, ds++) {
                spos = align_up(spos, 16);
                cl.val_off = spos;
                spos += align_up((uint64_t)st.nodes[lk.key_column][sc.chunk].n.n_present * 8, 16);
                h_colloc[(uint64_t)gi * n_proj + g->dslots[ds].proj] = cl;
            }
        }
        for (size_t e = 0; e < g->eslots.size(); e++) {
            /* a computed column reads as a sparse I64 column in scratch, laid
             * out like a derived one; expr_eval_kernel writes its bitmap
             * (zero here), rank words and values (exprs_build) */
            ColLoc cl{};
            cl.type = CSTRIPE_I64;
            cl.width = 8;
            cl.flags = 1;
            dpos = align_up(dpos, 8);
            cl.exists_off = dpos;
            dpos += align_up((rows + 7) / 8, 8);
            cl.rank_off = (uint32_t)h_rank.size();
            h_rank.resize(h_rank.size() + (rows + 63) / 64, 0);
            spos = align_up(spos, 16);
            cl.val_off = spos;
            spos += align_up((uint64_t)rows * 8, 16);
            h_colloc[(uint64_t)gi * n_proj + g->eslots[e]] = cl;
        }
    }

    /* invariant: the layout pass and the fill pass must agree exactly —
     * any drift between them is silent corruption (heap overflow on the
     * host copy or device reads past staged regions) */
    if (align_up(dpos, 16) > data_bytes || align_up(spos, 16) > scratch_bytes + 15 ||
        h_rank.size() > rank_words) {
        cs_set_err("staging layout drift: filled %llu/%llu data, %llu/%llu scratch, %llu/%llu rank words",
                   (unsigned long long)dpos, (unsigned long long)data_bytes,
                   (unsigned long long)spos, (unsigned long long)scratch_bytes,
                   (unsigned long long)h_rank.size(), (unsigned long long)rank_words);
        csgpu_release(s);
        return CSTRIPE_ERR;
    }
    HIP_TRY(hipMemcpyAsync(g->d_data, h_data.data(), data_bytes, hipMemcpyHostToDevice, g->stream));
    if (!h_rank.empty())
        HIP_TRY(hipMemcpyAsync(g->d_rank, h_rank.data(), h_rank.size() * 4, hipMemcpyHostToDevice, g->stream));
    if (!h_segs.empty())
        HIP_TRY(hipMemcpyAsync(g->d_segs, h_segs.data(), h_segs.size() * sizeof(SegDesc), hipMemcpyHostToDevice, g->stream));
    if (!h_zsegs.empty()) {
        /* sort frames by compressed length so a wave's 64 lanes decode
         * similar-cost frames: the serial FSE decode runs in lockstep per
         * wave (and per block up to the flush barrier), so one expensive
         * frame otherwise gates 127 cheap ones (frames are independent —
         * dst_off travels with the descriptor) */
        std::stable_sort(h_zsegs.begin(), h_zsegs.end(),
                         [](const SegDesc &a, const SegDesc &b) {
                             return a.comp_len > b.comp_len;
                         });
        HIP_TRY(hipMemcpyAsync(g->d_zsegs, h_zsegs.data(), h_zsegs.size() * sizeof(SegDesc), hipMemcpyHostToDevice, g->stream));
        static zr_dtables h_zrtab;
        static bool zrtab_init = false;
        if (!zrtab_init) { zr_build_dtables(&h_zrtab); zrtab_init = true; }
        HIP_TRY(hipMemcpyAsync(g->d_zrtab, &h_zrtab, sizeof(h_zrtab), hipMemcpyHostToDevice, g->stream));
    }
    HIP_TRY(hipMemcpyAsync(g->d_groups, h_groups.data(), h_groups.size() * sizeof(GroupDesc), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->d_colloc, h_colloc.data(), h_colloc.size() * sizeof(ColLoc), hipMemcpyHostToDevice, g->stream));
    if (g->fusable && g->n_groups > 0) {
        std::vector<FusedTile> h_tiles;
        h_tiles.reserve(n_tiles_max);
        for (uint32_t gi = 0; gi < g->n_groups; gi++) {
            const cs_selchunk &sc = s->sel[gi];
            uint32_t rows = r->stripes[sc.stripe].group_rows[sc.chunk];
            uint32_t ntile = (rows + FUSE_TILE_ROWS - 1) / FUSE_TILE_ROWS;
            for (uint32_t k = 0; k < ntile; k++) {
                FusedTile ft{};
                ft.row_count = (k + 1 < ntile) ? FUSE_TILE_ROWS
                                               : rows - k * FUSE_TILE_ROWS;
                for (uint32_t pj = 0; pj < n_proj; pj++)
                    ft.seg_base[pj] = seg_start[(uint64_t)gi * n_proj + pj] + 64 * k;
                h_tiles.push_back(ft);
            }
        }
        g->n_tiles = (uint32_t)h_tiles.size();
        HIP_TRY(hipMalloc(&g->d_tiles, h_tiles.size() * sizeof(FusedTile)));
        HIP_TRY(hipMemcpyAsync(g->d_tiles, h_tiles.data(),
                               h_tiles.size() * sizeof(FusedTile),
                               hipMemcpyHostToDevice, g->stream));
    }
    HIP_TRY(hipStreamSynchronize(g->stream));
    /* which projected columns the overlapped dense body can read: one pass
     * over the descriptors just built */
    g->col_ov.assign(n_proj, 1);
    g->any_zr = false;
    for (uint64_t i = 0; i < h_colloc.size(); i++) {
        const ColLoc &cl = h_colloc[i];
        if (cl.mode >= CSF_SEGMODE_ZRP_BASE) g->any_zr = true;
        const bool shape =
            cl.mode == CSF_SEGMODE_CONST || cl.mode == CSF_SEGMODE_ZR_CONST ||
            (((cl.mode & 0xF0u) == CSF_SEGMODE_P_BASE ||
              (cl.mode & 0xF0u) == CSF_SEGMODE_ZRP_BASE) &&
             (cl.mode & 0xFu) >= 1 && (cl.mode & 0xFu) <= 4 && cl.L == (cl.mode & 0xFu));
        if (!((cl.flags & 2) && (cl.flags & 4) && !(cl.flags & 1) &&
              cl.type == CSTRIPE_I64 && shape))
            g->col_ov[i % n_proj] = 0;
    }
    g->max_group_rows = 0;
    for (const GroupDesc &gd : h_groups)
        if (gd.row_count > g->max_group_rows) g->max_group_rows = gd.row_count;
    if (hipDeviceGetAttribute(&g->n_cus, hipDeviceAttributeMultiprocessorCount,
                              g->device) != hipSuccess || g->n_cus <= 0)
        g->n_cus = 256;
    g->colloc_host = h_colloc;
    s->text_dicts.clear();
    s->last_text_decode_ms = s->last_text_walk_ms = 0;
    s->last_text_dict_ms = s->last_text_remap_ms = 0;
    g->tpred_op.assign(s->preds.size(), 0);
    g->tpred_ival.assign(s->preds.size(), 0);
    if (any_vartext) {
        VtTemps vt;
        int rc = vartext_build(s, vt);
        vt.release();
        if (rc != CSTRIPE_OK) {
            /* the message is set; the scan is left unstaged */
            csgpu_release(s);
            s->text_dicts.clear();
            return rc;
        }
    }
    s->last_set_build_ms = s->last_set_probe_ms = 0;
    bool any_set_slot = false;
    for (const auto &ms : g->mslots) any_set_slot |= !ms.like;
    if (any_set_slot) {
        VtTemps st;
        int rc = sets_build(s, st);
        st.release();
        if (rc != CSTRIPE_OK) {
            csgpu_release(s);
            s->text_dicts.clear();
            return rc;
        }
    }
    s->last_lookup_build_ms = s->last_lookup_probe_ms = 0;
    if (!g->dslots.empty()) {
        VtTemps lt;
        int rc = lookups_build(s, lt);
        lt.release();
        if (rc != CSTRIPE_OK) {
            csgpu_release(s);
            s->text_dicts.clear();
            return rc;
        }
    }
    s->last_expr_ms = 0;
    if (!g->eslots.empty()) {
        VtTemps et;
        int rc = exprs_build(s, et);
        et.release();
        if (rc != CSTRIPE_OK) {
            csgpu_release(s);
            s->text_dicts.clear();
            return rc;
        }
    }
    return CSTRIPE_OK;
}

/* launch the decode grid: LDS-staged variant when every segment fits the
 * 64 KiB budget (writer default 8 KiB segments -> ~9 waves/CU), else the
 * global-memory fallback */
struct DecodeJob {
    const uint8_t *data;        /* staged compressed bytes (SegDesc.src_off) */
    uint8_t *out;               /* decode target (SegDesc.dst_off) */
    const SegDesc *segs;        /* LZ4 segments */
    uint32_t n_segs, max_seg_comp, max_seg_dlen;
    bool segs_16aligned;
    const SegDesc *zsegs;       /* restricted-zstd frames */
    uint32_t n_zsegs, max_zseg_comp, max_zseg_dlen;
};

static int launch_decode_job(cs_gpu_state *g, const DecodeJob &j)
{
    if (j.n_zsegs > 0) {
        /* CSTRIPE_ZR_VARIANT: 0 = force global kernel (A/B knob), default =
         * LDS-staged when the largest frame fits the budget */
        const char *zv = getenv("CSTRIPE_ZR_VARIANT");
        const int force = zv ? atoi(zv) : -1;
        /* stride: largest frame + 8 B slack (the aligned bit window and the
         * funnel loads may read a few bytes past comp_len, into the lane's
         * own slack), 16-aligned; tweaked off bank-aligned lane spacing */
        /* strides in ODD dword counts: lane l's frame starts at l*stride, so
         * equal-progress lanes hit bank (l*stride/4 + c) mod 64 — an odd
         * dword stride makes those 64 distinct banks (even residues conflict
         * 2-32 way; same rule as the lz4 lane kernel's 276/532/1044) */
        uint32_t stride = ((j.max_zseg_comp + 8 + 3) & ~3u) + 4;
        if (((stride / 4) & 1) == 0) stride += 4;
        uint32_t ostride = ((j.max_zseg_dlen + 3) & ~3u) + 4;
        if (((ostride / 4) & 1) == 0) ostride += 4;
        const uint32_t grid = (j.n_zsegs + ZR_LDS_BLOCK - 1) / ZR_LDS_BLOCK;
        const size_t lds1 = (size_t)ZR_LDS_BLOCK * stride + sizeof(zr_dtables);
        const size_t lds2 = lds1 + (size_t)ZR_LDS_BLOCK * ostride;
        if ((force == -1 || force >= 2) && lds2 <= 152 * 1024) {
            hipLaunchKernelGGL(zr_decode_lds2_kernel, dim3(grid), dim3(ZR_LDS_BLOCK),
                               lds2, g->stream,
                               j.data, j.out, j.zsegs, j.n_zsegs,
                               stride, ostride, g->d_zrtab, g->d_error);
        } else if (force != 0 && lds1 <= 152 * 1024) {
            hipLaunchKernelGGL(zr_decode_lds_kernel, dim3(grid), dim3(ZR_LDS_BLOCK),
                               lds1, g->stream,
                               j.data, j.out, j.zsegs, j.n_zsegs,
                               stride, g->d_zrtab, g->d_error);
        } else {
            const uint32_t grid = (j.n_zsegs + 255) / 256;
            hipLaunchKernelGGL(zr_decode_kernel, dim3(grid), dim3(256), 0, g->stream,
                               j.data, j.out, j.zsegs, j.n_zsegs,
                               g->d_zrtab, g->d_error);
        }
        HIP_TRY(hipGetLastError());
    }
    if (j.n_segs == 0) return CSTRIPE_OK;
    /* lane-parallel path for micro-segments (one lane per segment).
     * stride: 16 B-multiple, (stride/4)%64 != 0 so equal-progress lanes land
     * on different banks; LDS/wave = 64*stride -> waves/CU 9 / 4 / 2. */
    if (j.segs_16aligned && j.max_seg_dlen <= 1039) {
        uint32_t block, stride;
        if (j.max_seg_dlen <= 275)      { block = 256; stride = 276; }
        else if (j.max_seg_dlen <= 531) { block = 256; stride = 532; }
        else                             { block = 128; stride = 1044; }
        uint32_t grid = (j.n_segs + block - 1) / block;
        hipLaunchKernelGGL(lz4_decode_lane_kernel, dim3(grid), dim3(block),
                           block * stride + block * 16, g->stream,
                           j.data, j.out, j.segs, j.n_segs, stride,
                           g->d_error);
        HIP_TRY(hipGetLastError());
        return CSTRIPE_OK;
    }
    uint32_t in_cap = (j.max_seg_comp + 8 + 15) & ~15u;
    uint32_t out_cap = (j.max_seg_dlen + 15) & ~15u;
    if (in_cap + out_cap <= 64 * 1024) {
        hipLaunchKernelGGL(lz4_decode_lds_kernel, dim3(j.n_segs), dim3(WAVE),
                           in_cap + out_cap, g->stream,
                           j.data, j.out, j.segs, in_cap, g->d_error);
    } else {
        hipLaunchKernelGGL(lz4_decode_kernel, dim3(j.n_segs), dim3(WAVE), 0, g->stream,
                           j.data, j.out, j.segs, g->d_error);
    }
    /* a failed launch would leave d_scratch stale while later memcpys
       succeed -> silent garbage; surface it as an error (round-1 advisor) */
    HIP_TRY(hipGetLastError());
    return CSTRIPE_OK;
}

/* the scan's own decode grid: every staged LZ4 / restricted-zstd segment of
 * the fixed-width columns into d_scratch */
static int launch_decode(cs_gpu_state *g)
{
    DecodeJob j{g->d_data, g->d_scratch, g->d_segs, g->n_segs, g->max_seg_comp,
                g->max_seg_dlen, g->segs_16aligned, g->d_zsegs, g->n_zsegs,
                g->max_zseg_comp, g->max_zseg_dlen};
    return launch_decode_job(g, j);
}

/* =====================================================================
 * VARTEXT — variable-length text through a per-scan device dictionary.
 *
 * The varlena branch of DeserializeDatumArray (columnar_reader.c:1559-1565:
 * fetch_att / att_addlength_datum / att_align_nominal, one dependent step
 * per datum) run once per stage instead of once per row per query. For each
 * projected VARTEXT column, over the scan's SELECTED chunk groups:
 *   decode   the chunks' streams into a temporary buffer — the same LZ4 /
 *            restricted-zstd decode kernels over a SEPARATE segment list, so
 *            the per-call launch_decode of the query paths never touches
 *            text; NONE and host-decoded zstd/pglz chunks are staged raw
 *   walk     vt_walk_kernel: one wave per chunk-column; windows of the
 *            stream are staged into LDS with coalesced loads, lane 0 walks
 *            the headers at LDS latency (csvt_step, vartext.h), the wave
 *            writes (offset, length) words out coalesced. Bounded by the
 *            chunk's decompressed_size; overrun / miscount raises a flag
 *   dict     vt_dict_kernel: every value hashes its payload into a global
 *            open-addressing table; an EMPTY slot is claimed by one
 *            atomicCAS that stores a reference to the claimer's bytes
 *            (immutable since the walk), a loser compares bytes and adopts
 *            the slot or probes on; winners also reserve their place in the
 *            compact entry list and in the gather buffer
 *   gather   vt_gather_kernel: entry records + representative strings into
 *            one buffer, one DtoH copy; the host sorts by memcmp and uploads
 *            a slot -> rank table
 *   remap    vt_remap_kernel: int32 ranks into the column's scratch region
 * After that the column is a dense/sparse I32 column to every query kernel.
 * ===================================================================== */

#define VT_WIN      8192u   /* stream bytes per LDS window (multiple of 4) */
#define VT_OUT      1024u   /* values buffered per window */
#define VT_EMPTY    (~0ull)
#define VT_ERR_WALK     256
#define VT_ERR_DISTINCT 512

struct VtChunk {
    uint64_t raw_off;       /* decoded stream in the temp buffer, 16 B-aligned */
    uint64_t val_base;      /* index of the chunk's first value in vpos */
    uint64_t rank_off;      /* into d_scratch: n_present int32 ranks */
    uint32_t raw_len;       /* decompressed_size — the walk's bound */
    uint32_t n_present;
};

/* a value reference: payload offset in the temp buffer << 16 | length
 * (<= CSTRIPE_VARTEXT_MAX_LEN, checked by csvt_step); never VT_EMPTY */
struct VtEntry {
    unsigned long long ref;
    unsigned long long boff;    /* byte offset of the copy in the gather buffer */
    uint32_t slot;
    uint32_t pad;
};

__global__ __launch_bounds__(WAVE) void vt_walk_kernel(
    const uint8_t *__restrict__ raw, const VtChunk *__restrict__ chunks,
    unsigned long long *__restrict__ vpos, int *__restrict__ err)
{
    __shared__ __attribute__((aligned(16))) uint8_t win[VT_WIN];
    __shared__ unsigned long long outb[VT_OUT];
    __shared__ uint32_t s_n, s_adv, s_bad;
    const VtChunk ck = chunks[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint64_t len = ck.raw_len;
    uint64_t pos = 0;               /* always 4-aligned: datums are padded */
    uint32_t count = 0;
    bool bad = false;
    while (pos < len && count < ck.n_present && !bad) {
        const uint32_t wlen = (uint32_t)min((uint64_t)VT_WIN, len - pos);
        /* raw_off is 16-aligned and the buffer ends in slack, so whole
         * dwords load even when wlen is not a multiple of 4 */
        const uint32_t *src = (const uint32_t *)(raw + ck.raw_off + pos);
        for (uint32_t i = lane; i < (wlen + 3) / 4; i += WAVE)
            ((uint32_t *)win)[i] = src[i];
        __syncthreads();
        if (lane == 0) {
            uint32_t w = 0, n = 0, e = 0;
            /* w < wlen and w 4-aligned: a 4-byte header csvt_step reads
             * (only when >= 4 stream bytes remain) lies inside the window */
            while (w < wlen && n < VT_OUT && count + n < ck.n_present) {
                uint32_t po, pl, adv;
                if (csvt_step(win + w, len - (pos + w), &po, &pl, &adv)) { e = 1; break; }
                outb[n++] = ((unsigned long long)(ck.raw_off + pos + w + po) << 16) | pl;
                w += adv;           /* past wlen when the datum outgrows the
                                     * window: the next window starts there */
            }
            s_n = n; s_adv = w; s_bad = e;
        }
        __syncthreads();
        const uint32_t n = s_n;
        for (uint32_t i = lane; i < n; i += WAVE)
            vpos[ck.val_base + count + i] = outb[i];
        count += n;
        pos += s_adv;
        bad = s_bad != 0;
        __syncthreads();
    }
    if (lane == 0 && (bad || count != ck.n_present || pos < len))
        atomicOr(err, VT_ERR_WALK);
}

__device__ inline uint64_t vt_hash(const uint8_t *p, uint32_t len)
{
    uint64_t h = 0xcbf29ce484222325ull;             /* FNV-1a, then a finalizer */
    for (uint32_t i = 0; i < len; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    return h;
}

__global__ __launch_bounds__(AGG_BLOCK) void vt_dict_kernel(
    const uint8_t *__restrict__ raw, const unsigned long long *__restrict__ vpos,
    uint64_t n_values, unsigned long long *table, uint64_t slots,
    uint32_t *__restrict__ vslot, VtEntry *__restrict__ entries,
    unsigned long long *counters, uint32_t max_distinct, int *err)
{
    const uint64_t mask = slots - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; i < n_values;
         i += (uint64_t)gridDim.x * AGG_BLOCK) {
        const unsigned long long ref = vpos[i];
        const uint8_t *p = raw + (ref >> 16);
        const uint32_t len = (uint32_t)(ref & 0xFFFFu);
        uint64_t slot = vt_hash(p, len) & mask;
        bool found = false;
        for (uint64_t probe = 0; probe < slots && !found; probe++) {
            /* look before claiming: a column of few distinct values would
             * otherwise send every row's CAS to the same few addresses */
            unsigned long long cur = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
            if (cur == VT_EMPTY) {
                cur = atomicCAS(&table[slot], VT_EMPTY, ref);
                if (cur == VT_EMPTY) {      /* claimed: this value represents the slot */
                    const unsigned long long e = atomicAdd(&counters[0], 1ull);
                    if (e >= max_distinct) {
                        atomicOr(err, VT_ERR_DISTINCT);
                    } else {
                        VtEntry en;
                        en.ref = ref;
                        en.boff = atomicAdd(&counters[1], (unsigned long long)len);
                        en.slot = (uint32_t)slot;
                        en.pad = 0;
                        entries[e] = en;
                    }
                    found = true;
                    break;
                }
            }
            /* occupied: the winner's bytes were written by an earlier kernel,
             * so comparing them needs no flag or fence */
            if ((uint32_t)(cur & 0xFFFFu) == len) {
                const uint8_t *q = raw + (cur >> 16);
                uint32_t k = 0;
                while (k < len && p[k] == q[k]) k++;
                if (k == len) { found = true; break; }
            }
            slot = (slot + 1) & mask;
            if ((probe & 63u) == 63u &&
                (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & VT_ERR_DISTINCT))
                break;                      /* the stage fails anyway */
        }
        if (!found) { atomicOr(err, VT_ERR_DISTINCT); slot = 0; }
        vslot[i] = (uint32_t)slot;
    }
}

/* out = [n_dict VtEntry records][representative strings at boff] */
__global__ __launch_bounds__(AGG_BLOCK) void vt_gather_kernel(
    const uint8_t *__restrict__ raw, const VtEntry *__restrict__ entries,
    uint32_t n_dict, uint8_t *__restrict__ out)
{
    uint8_t *obytes = out + (uint64_t)n_dict * sizeof(VtEntry);
    for (uint32_t e = blockIdx.x * AGG_BLOCK + threadIdx.x; e < n_dict;
         e += gridDim.x * AGG_BLOCK) {
        const VtEntry en = entries[e];
        ((VtEntry *)out)[e] = en;
        const uint8_t *p = raw + (en.ref >> 16);
        const uint32_t len = (uint32_t)(en.ref & 0xFFFFu);
        uint8_t *d = obytes + en.boff;
        for (uint32_t k = 0; k < len; k++) d[k] = p[k];
    }
}

/* one block per chunk-column of the column being remapped */
__global__ __launch_bounds__(AGG_BLOCK) void vt_remap_kernel(
    const VtChunk *__restrict__ chunks, const uint32_t *__restrict__ vslot,
    uint64_t vbeg, const uint32_t *__restrict__ slot2rank, uint8_t *__restrict__ scratch)
{
    const VtChunk ck = chunks[blockIdx.x];
    int32_t *dst = (int32_t *)(scratch + ck.rank_off);
    const uint32_t *vs = vslot + (ck.val_base - vbeg);
    for (uint32_t i = threadIdx.x; i < ck.n_present; i += AGG_BLOCK)
        dst[i] = (int32_t)slot2rank[vs[i]];
}

/* ---- LIKE / NOT LIKE (cstripe.h): the pattern travels by value in the
 * kernel argument; one lane matches one value with cslk_match (like.h), whose
 * reads stay inside [ref >> 16, +len) of the temp buffer — bounds the walk
 * checked. Lanes of a wave diverge on value length; long values are not
 * split across lanes. ---- */
struct LikePat {
    uint32_t len;
    uint8_t b[CSLK_MAX_PATTERN];
};

#define VT_LIKE_VALS 4u                         /* values per lane */
#define VT_LIKE_TILE (AGG_BLOCK * VT_LIKE_VALS)

/* DICT form: one lane per dictionary entry, a 0/1 byte per table slot */
__global__ __launch_bounds__(AGG_BLOCK) void vt_like_kernel(
    const uint8_t *__restrict__ raw, const VtEntry *__restrict__ entries,
    uint32_t n_dict, uint8_t *__restrict__ flag, const LikePat pat)
{
    for (uint32_t e = blockIdx.x * AGG_BLOCK + threadIdx.x; e < n_dict;
         e += gridDim.x * AGG_BLOCK) {
        const VtEntry en = entries[e];
        flag[en.slot] = (uint8_t)cslk_match(pat.b, pat.len, raw + (en.ref >> 16),
                                            (uint32_t)(en.ref & 0xFFFFu));
    }
}

/* DICT form: one block per chunk-column, member[i] = flag[vslot[i]]; lane:
 * four consecutive values, one dword of 0/1 bytes. The member region is
 * padded to 16 bytes, so the tail dword stays inside it. */
__global__ __launch_bounds__(AGG_BLOCK) void vt_like_apply_kernel(
    const VtChunk *__restrict__ chunks, const uint64_t *__restrict__ member_off,
    const uint32_t *__restrict__ vslot, uint64_t vbeg, const uint8_t *__restrict__ flag,
    uint8_t *__restrict__ scratch)
{
    const VtChunk ck = chunks[blockIdx.x];
    uint8_t *dst = scratch + member_off[blockIdx.x];
    const uint32_t *vs = vslot + (ck.val_base - vbeg);
    for (uint32_t v0 = threadIdx.x * VT_LIKE_VALS; v0 < ck.n_present; v0 += VT_LIKE_TILE) {
        uint32_t word = 0;
        #pragma unroll
        for (uint32_t k = 0; k < VT_LIKE_VALS; k++)
            if (v0 + k < ck.n_present) word |= (uint32_t)flag[vs[v0 + k]] << (8u * k);
        *(uint32_t *)(dst + v0) = word;
    }
}

/* STREAM form: one block per (chunk-column, tile of VT_LIKE_TILE values),
 * matching straight off the walk's (offset, length) words; the same lane
 * shape and store as above */
__global__ __launch_bounds__(AGG_BLOCK) void vt_like_stream_kernel(
    const uint8_t *__restrict__ raw, const unsigned long long *__restrict__ vpos,
    const VtChunk *__restrict__ chunks, const uint64_t *__restrict__ member_off,
    uint32_t tiles_pc, uint8_t *__restrict__ scratch, const LikePat pat)
{
    const uint32_t ci = blockIdx.x / tiles_pc, tile = blockIdx.x % tiles_pc;
    const VtChunk ck = chunks[ci];
    const uint32_t v0 = (tile * AGG_BLOCK + threadIdx.x) * VT_LIKE_VALS;
    if (v0 >= ck.n_present) return;
    uint32_t word = 0;
    #pragma unroll
    for (uint32_t k = 0; k < VT_LIKE_VALS; k++) {
        if (v0 + k >= ck.n_present) break;
        const unsigned long long ref = vpos[ck.val_base + v0 + k];
        word |= (uint32_t)cslk_match(pat.b, pat.len, raw + (ref >> 16),
                                     (uint32_t)(ref & 0xFFFFu)) << (8u * k);
    }
    *(uint32_t *)(scratch + member_off[ci] + v0) = word;
}

/* memcmp order, the shorter string first on a prefix tie */
static inline int vt_cmp(const uint8_t *a, size_t al, const uint8_t *b, size_t bl)
{
    const int c = memcmp(a, b, al < bl ? al : bl);
    if (c) return c;
    return al < bl ? -1 : (al > bl ? 1 : 0);
}

static int vartext_build(cstripe_scan *s, VtTemps &vt)
{
    cs_gpu_state *g = s->gpu;
    cstripe_reader *r = s->r;
    const uint32_t n_cols = r->head.column_count, n_proj = g->n_proj;
    s->text_dicts.assign(n_cols, cs_text_dict());
    std::vector<uint32_t> vcols;
    for (uint32_t c = 0; c < n_cols; c++)
        if (g->proj_of_col[c] >= 0 && r->cols[c].type == CSTRIPE_VARTEXT) vcols.push_back(c);

    uint32_t max_distinct = CSTRIPE_VARTEXT_MAX_DISTINCT;
    if (const char *e = getenv("CSTRIPE_VARTEXT_MAX_DISTINCT")) {
        const long v = atol(e);
        if (v >= 1 && (unsigned long)v < max_distinct) max_distinct = (uint32_t)v;
    }

    /* ---- layout: chunk-columns column-major, their streams and segments ---- */
    enum { K_RAW, K_LZ4, K_ZR, K_HOST };
    std::vector<VtChunk> chunks;
    std::vector<uint8_t> kinds;
    std::vector<uint64_t> comp_off;
    std::vector<uint64_t> col_cbeg(vcols.size() + 1, 0), col_vbeg(vcols.size() + 1, 0);
    uint64_t comp_bytes = 0, raw_bytes = 0, n_values = 0;
    bool any_host_raw = false;
    for (size_t ci = 0; ci < vcols.size(); ci++) {
        const uint32_t c = vcols[ci];
        col_cbeg[ci] = chunks.size();
        col_vbeg[ci] = n_values;
        for (uint32_t gi = 0; gi < g->n_groups; gi++) {
            const cs_selchunk &sc = s->sel[gi];
            const cs_skipnode &nd = r->stripes[sc.stripe].nodes[c][sc.chunk];
            if (nd.n.decompressed_size >= (1ull << 32) || nd.n.n_present > nd.n.row_count) {
                cs_set_err("VARTEXT column %u: bad chunk sizes in the footer", c);
                return CSTRIPE_ERR_FORMAT;
            }
            uint8_t kind = K_HOST;
            if (nd.n.comp_type == CSTRIPE_COMP_NONE) kind = K_RAW;
            else if (nd.n.comp_type == CSTRIPE_COMP_LZ4) kind = K_LZ4;
            else if (nd.n.comp_type == CSTRIPE_COMP_ZSTD) {
                kind = K_ZR;
                for (uint8_t m : nd.seg_modes)
                    if (m != CSF_SEGMODE_ZR) { kind = K_HOST; break; }
            } else if (nd.n.comp_type != CSTRIPE_COMP_PGLZ) {
                cs_set_err("unsupported chunk compression %d", nd.n.comp_type);
                return CSTRIPE_ERR_FORMAT;
            }
            if (kind == K_RAW && nd.n.value_len != nd.n.decompressed_size) {
                cs_set_err("VARTEXT column %u: uncompressed chunk of %llu bytes claims %llu",
                           c, (unsigned long long)nd.n.value_len,
                           (unsigned long long)nd.n.decompressed_size);
                return CSTRIPE_ERR_FORMAT;
            }
            /* the decoders write [decomp_off, +decomp_len) of the chunk's
             * region: keep every segment inside it */
            for (const csf_seg &sg : nd.segs)
                if ((uint64_t)sg.decomp_off + sg.decomp_len > nd.n.decompressed_size ||
                    (uint64_t)sg.comp_off + sg.comp_len > nd.n.value_len) {
                    cs_set_err("VARTEXT column %u: segment outside its chunk", c);
                    return CSTRIPE_ERR_FORMAT;
                }
            VtChunk ck{};
            ck.raw_off = raw_bytes;
            ck.raw_len = (uint32_t)nd.n.decompressed_size;
            ck.n_present = nd.n.n_present;
            ck.val_base = n_values;
            ck.rank_off = g->colloc_host[(uint64_t)gi * n_proj + g->proj_of_col[c]].val_off;
            raw_bytes += align_up(nd.n.decompressed_size, 16);
            n_values += nd.n.n_present;
            comp_off.push_back(comp_bytes);
            if (kind == K_LZ4 || kind == K_ZR) comp_bytes += align_up(nd.n.value_len, 16);
            else any_host_raw = true;
            chunks.push_back(ck);
            kinds.push_back(kind);
        }
    }
    col_cbeg[vcols.size()] = chunks.size();
    col_vbeg[vcols.size()] = n_values;
    for (size_t ci = 0; ci < vcols.size(); ci++) {
        /* a STREAM-form column gets no dictionary (cstripe_scan_text_dict) */
        s->text_dicts[vcols[ci]].built = g->like_form[vcols[ci]] != CSTRIPE_LIKE_FORM_STREAM;
        s->text_dicts[vcols[ci]].offsets.assign(1, 0);
    }

    if (!chunks.empty()) {
        /* ---- fill the host staging buffers ---- */
        std::vector<uint8_t> h_comp(comp_bytes, 0);
        std::vector<uint8_t> h_raw(any_host_raw ? raw_bytes : 0, 0);
        std::vector<SegDesc> lsegs, zsegs;
        DecodeJob job{};
        job.segs_16aligned = true;
        size_t k = 0;
        for (size_t ci = 0; ci < vcols.size(); ci++) {
            const uint32_t c = vcols[ci];
            for (uint32_t gi = 0; gi < g->n_groups; gi++, k++) {
                const cs_selchunk &sc = s->sel[gi];
                const cs_stripe_info &st = r->stripes[sc.stripe];
                const cs_skipnode &nd = st.nodes[c][sc.chunk];
                const uint8_t *src = r->stripe_base(st) + nd.n.value_off;
                const VtChunk &ck = chunks[k];
                if (kinds[k] == K_RAW) {
                    memcpy(h_raw.data() + ck.raw_off, src, nd.n.value_len);
                } else if (kinds[k] == K_HOST) {
                    for (const csf_seg &sg : nd.segs) {
                        uint8_t *dst = h_raw.data() + ck.raw_off + sg.decomp_off;
                        if (nd.n.comp_type == CSTRIPE_COMP_ZSTD) {
                            const size_t zr = ZSTD_decompress(dst, sg.decomp_len, src + sg.comp_off, sg.comp_len);
                            if (ZSTD_isError(zr) || zr != sg.decomp_len) { cs_set_err("zstd host decode failed"); return CSTRIPE_ERR_FORMAT; }
                        } else {
                            const uint8_t *pb = src + sg.comp_off;
                            if (sg.comp_len < CSPGLZ_HDRSZ ||
                                cspglz_varsize(pb) != sg.comp_len ||
                                cspglz_rawsize(pb) != (int32_t)sg.decomp_len ||
                                cspglz_decompress(pb + CSPGLZ_HDRSZ, (int32_t)(sg.comp_len - CSPGLZ_HDRSZ),
                                                  dst, (int32_t)sg.decomp_len) < 0) {
                                cs_set_err("pglz host decode failed");
                                return CSTRIPE_ERR_FORMAT;
                            }
                        }
                    }
                } else {
                    memcpy(h_comp.data() + comp_off[k], src, nd.n.value_len);
                    for (const csf_seg &sg : nd.segs) {
                        SegDesc sd;
                        sd.src_off = comp_off[k] + sg.comp_off;
                        sd.dst_off = ck.raw_off + sg.decomp_off;
                        sd.comp_len = sg.comp_len;
                        sd.decomp_len = sg.decomp_len;
                        if (kinds[k] == K_LZ4) {
                            job.max_seg_comp = std::max(job.max_seg_comp, sg.comp_len);
                            job.max_seg_dlen = std::max(job.max_seg_dlen, sg.decomp_len);
                            if (sg.decomp_off % 16 != 0) job.segs_16aligned = false;
                            lsegs.push_back(sd);
                        } else {
                            job.max_zseg_comp = std::max(job.max_zseg_comp, sg.comp_len);
                            job.max_zseg_dlen = std::max(job.max_zseg_dlen, sg.decomp_len);
                            zsegs.push_back(sd);
                        }
                    }
                }
            }
        }
        std::stable_sort(zsegs.begin(), zsegs.end(),
                         [](const SegDesc &a, const SegDesc &b) { return a.comp_len > b.comp_len; });

        /* ---- device buffers (+256: the decoders' and the walk's whole-word
         * reads reach a few bytes past a region's end) ---- */
        uint8_t *t_comp = nullptr, *t_raw = nullptr;
        VtChunk *d_chunks = nullptr;
        SegDesc *d_lsegs = nullptr, *d_zs = nullptr;
        unsigned long long *d_vpos = nullptr;
        HIP_TRY(vt.alloc(t_comp, comp_bytes + 256));
        HIP_TRY(vt.alloc(t_raw, raw_bytes + 256));
        HIP_TRY(vt.alloc(d_chunks, chunks.size() * sizeof(VtChunk)));
        HIP_TRY(vt.alloc(d_lsegs, lsegs.size() * sizeof(SegDesc)));
        HIP_TRY(vt.alloc(d_zs, zsegs.size() * sizeof(SegDesc)));
        HIP_TRY(vt.alloc(d_vpos, n_values * sizeof(unsigned long long)));
        for (hipEvent_t &e : vt.ev) HIP_TRY(hipEventCreate(&e));
        if (any_host_raw)
            HIP_TRY(hipMemcpyAsync(t_raw, h_raw.data(), raw_bytes, hipMemcpyHostToDevice, g->stream));
        else
            HIP_TRY(hipMemsetAsync(t_raw + raw_bytes, 0, 256, g->stream));
        if (comp_bytes)
            HIP_TRY(hipMemcpyAsync(t_comp, h_comp.data(), comp_bytes, hipMemcpyHostToDevice, g->stream));
        HIP_TRY(hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(VtChunk), hipMemcpyHostToDevice, g->stream));
        if (!lsegs.empty())
            HIP_TRY(hipMemcpyAsync(d_lsegs, lsegs.data(), lsegs.size() * sizeof(SegDesc), hipMemcpyHostToDevice, g->stream));
        if (!zsegs.empty()) {
            HIP_TRY(hipMemcpyAsync(d_zs, zsegs.data(), zsegs.size() * sizeof(SegDesc), hipMemcpyHostToDevice, g->stream));
            if (!g->d_zrtab) {      /* no fixed-width column brought the tables */
                static zr_dtables h_zrtab2;
                static bool zrtab2_init = false;
                if (!zrtab2_init) { zr_build_dtables(&h_zrtab2); zrtab2_init = true; }
                HIP_TRY(hipMalloc(&g->d_zrtab, sizeof(zr_dtables)));
                HIP_TRY(hipMemcpyAsync(g->d_zrtab, &h_zrtab2, sizeof(h_zrtab2), hipMemcpyHostToDevice, g->stream));
            }
        }
        job.data = t_comp;
        job.out = t_raw;
        job.segs = d_lsegs;
        job.n_segs = (uint32_t)lsegs.size();
        job.zsegs = d_zs;
        job.n_zsegs = (uint32_t)zsegs.size();

        /* ---- decode + walk ---- */
        HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
        HIP_TRY(hipEventRecord(vt.ev[0], g->stream));
        { int _rc = launch_decode_job(g, job); if (_rc != CSTRIPE_OK) return _rc; }
        HIP_TRY(hipEventRecord(vt.ev[1], g->stream));
        hipLaunchKernelGGL(vt_walk_kernel, dim3((uint32_t)chunks.size()), dim3(WAVE), 0, g->stream,
                           t_raw, d_chunks, d_vpos, g->d_error);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(vt.ev[2], g->stream));
        int h_err = 0;
        HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, vt.ev[0], vt.ev[1]);
        s->last_text_decode_ms = ms;
        (void)hipEventElapsedTime(&ms, vt.ev[1], vt.ev[2]);
        s->last_text_walk_ms = ms;
        if (h_err & ~VT_ERR_WALK) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
        if (h_err & VT_ERR_WALK) {
            cs_set_err("VARTEXT stream malformed: a datum overruns its chunk or the datum "
                       "count differs from n_present (device flag %d)", h_err);
            return CSTRIPE_ERR_FORMAT;
        }

        /* the LIKE member slots of column vcols[ci], one pattern at a time:
         * STREAM (d_ent null) matches every value off d_vpos; DICT matches
         * the n_dict entries into a flag byte per table slot, then applies
         * the flags through d_vslot */
        auto like_build = [&](size_t ci, const VtEntry *d_ent, uint32_t n_dict, uint64_t slots,
                              const uint32_t *d_vslot) -> int {
            const uint32_t c = vcols[ci];
            const uint32_t ncks = (uint32_t)(col_cbeg[ci + 1] - col_cbeg[ci]);
            uint32_t max_np = 0;
            for (uint64_t k = col_cbeg[ci]; k < col_cbeg[ci + 1]; k++)
                max_np = std::max(max_np, chunks[k].n_present);
            const uint32_t tiles_pc = std::max(1u, (max_np + VT_LIKE_TILE - 1) / VT_LIKE_TILE);
            if ((uint64_t)ncks * tiles_pc >= (1ull << 31)) { cs_set_err("gpu_stage: too many tiles for the LIKE match"); return CSTRIPE_ERR_ARG; }
            for (const auto &ms : g->mslots) {
                if (!ms.like || ms.col != c) continue;
                const uint32_t mark = vt.n_bufs;
                const std::string &ptx = s->text_consts[ms.set];
                LikePat pat{};
                if (ptx.size() > CSLK_MAX_PATTERN) { cs_set_err("gpu_stage: LIKE pattern too long"); return CSTRIPE_ERR; }
                pat.len = (uint32_t)ptx.size();
                memcpy(pat.b, ptx.data(), ptx.size());
                std::vector<uint64_t> moff(ncks);
                for (uint32_t gi = 0; gi < ncks; gi++)
                    moff[gi] = g->colloc_host[(uint64_t)gi * n_proj + ms.proj].val_off;
                uint64_t *d_moff = nullptr;
                uint8_t *d_flag = nullptr;
                HIP_TRY(vt.alloc(d_moff, ncks * sizeof(uint64_t)));
                HIP_TRY(hipMemcpyAsync(d_moff, moff.data(), ncks * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream));
                if (d_ent) {
                    HIP_TRY(vt.alloc(d_flag, slots));
                    HIP_TRY(hipMemsetAsync(d_flag, 0, slots, g->stream));
                }
                HIP_TRY(hipEventRecord(vt.ev[3], g->stream));
                if (d_ent) {
                    if (n_dict)
                        hipLaunchKernelGGL(vt_like_kernel, dim3((n_dict + AGG_BLOCK - 1) / AGG_BLOCK),
                                           dim3(AGG_BLOCK), 0, g->stream, t_raw, d_ent, n_dict, d_flag, pat);
                } else {
                    hipLaunchKernelGGL(vt_like_stream_kernel, dim3(ncks * tiles_pc), dim3(AGG_BLOCK), 0,
                                       g->stream, t_raw, d_vpos, d_chunks + col_cbeg[ci], d_moff,
                                       tiles_pc, g->d_scratch, pat);
                }
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(vt.ev[4], g->stream));
                if (d_ent) {
                    hipLaunchKernelGGL(vt_like_apply_kernel, dim3(ncks), dim3(AGG_BLOCK), 0, g->stream,
                                       d_chunks + col_cbeg[ci], d_moff, d_vslot, col_vbeg[ci], d_flag,
                                       g->d_scratch);
                    HIP_TRY(hipGetLastError());
                }
                HIP_TRY(hipEventRecord(vt.ev[7], g->stream));
                HIP_TRY(hipStreamSynchronize(g->stream));
                float lms = 0;
                (void)hipEventElapsedTime(&lms, vt.ev[3], vt.ev[4]);
                s->last_like_match_ms += lms;
                if (d_ent) {
                    (void)hipEventElapsedTime(&lms, vt.ev[4], vt.ev[7]);
                    s->last_like_apply_ms += lms;
                }
                vt.free_from(mark);
            }
            return CSTRIPE_OK;
        };

        /* ---- per column: dictionary, gather, host sort, remap ---- */
        for (size_t ci = 0; ci < vcols.size(); ci++) {
            const uint32_t c = vcols[ci];
            const uint64_t vbeg = col_vbeg[ci], nv = col_vbeg[ci + 1] - vbeg;
            const uint32_t ncks = (uint32_t)(col_cbeg[ci + 1] - col_cbeg[ci]);
            if (nv == 0) continue;             /* all NULL: empty dictionary */
            if (g->like_form[c] == CSTRIPE_LIKE_FORM_STREAM) {
                /* only pattern-matched: no table, no gather, no sort, no ranks */
                { int _rc = like_build(ci, nullptr, 0, 0, nullptr); if (_rc != CSTRIPE_OK) return _rc; }
                continue;
            }
            const uint32_t mark = vt.n_bufs;
            const uint64_t cap = std::min<uint64_t>(max_distinct, nv);
            uint64_t slots = 2;
            while (slots < 2 * cap) slots <<= 1;
            unsigned long long *d_table = nullptr, *d_cnt = nullptr;
            uint32_t *d_vslot = nullptr, *d_s2r = nullptr;
            VtEntry *d_ent = nullptr;
            uint8_t *d_gather = nullptr;
            HIP_TRY(vt.alloc(d_table, slots * sizeof(unsigned long long)));
            HIP_TRY(vt.alloc(d_cnt, 2 * sizeof(unsigned long long)));
            HIP_TRY(vt.alloc(d_vslot, nv * sizeof(uint32_t)));
            HIP_TRY(vt.alloc(d_ent, cap * sizeof(VtEntry)));
            HIP_TRY(hipMemsetAsync(d_table, 0xFF, slots * sizeof(unsigned long long), g->stream));
            HIP_TRY(hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned long long), g->stream));
            const uint64_t vblocks = (nv + AGG_BLOCK - 1) / AGG_BLOCK;
            const uint32_t dgrid = (uint32_t)std::min<uint64_t>(vblocks, 65536);
            HIP_TRY(hipEventRecord(vt.ev[3], g->stream));
            hipLaunchKernelGGL(vt_dict_kernel, dim3(dgrid), dim3(AGG_BLOCK), 0, g->stream,
                               t_raw, d_vpos + vbeg, nv, d_table, slots, d_vslot, d_ent,
                               d_cnt, (uint32_t)cap, g->d_error);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(vt.ev[4], g->stream));
            unsigned long long h_cnt[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, g->stream));
            HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
            HIP_TRY(hipStreamSynchronize(g->stream));
            (void)hipEventElapsedTime(&ms, vt.ev[3], vt.ev[4]);
            s->last_text_dict_ms += ms;
            if (h_err & VT_ERR_DISTINCT) {
                cs_set_err("gpu_stage: VARTEXT column %u holds more than %u distinct values over "
                           "the selected chunk groups (CSTRIPE_VARTEXT_MAX_DISTINCT) — not "
                           "pushdownable through the device dictionary", c, max_distinct);
                return CSTRIPE_ERR_ARG;
            }
            const uint32_t n_dict = (uint32_t)h_cnt[0];
            const uint64_t n_bytes = h_cnt[1];
            const uint64_t gbytes = (uint64_t)n_dict * sizeof(VtEntry) + n_bytes;
            HIP_TRY(vt.alloc(d_gather, gbytes));
            HIP_TRY(hipEventRecord(vt.ev[3], g->stream));
            hipLaunchKernelGGL(vt_gather_kernel, dim3((n_dict + AGG_BLOCK - 1) / AGG_BLOCK),
                               dim3(AGG_BLOCK), 0, g->stream, t_raw, d_ent, n_dict, d_gather);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(vt.ev[4], g->stream));
            std::vector<uint8_t> h_g(gbytes);
            HIP_TRY(hipMemcpyAsync(h_g.data(), d_gather, gbytes, hipMemcpyDeviceToHost, g->stream));
            HIP_TRY(hipStreamSynchronize(g->stream));
            (void)hipEventElapsedTime(&ms, vt.ev[3], vt.ev[4]);
            s->last_text_dict_ms += ms;

            /* host sort by memcmp; ranks are positions in that order */
            const VtEntry *ents = (const VtEntry *)h_g.data();
            const uint8_t *gb = h_g.data() + (uint64_t)n_dict * sizeof(VtEntry);
            for (uint32_t e = 0; e < n_dict; e++)
                if (ents[e].boff + (ents[e].ref & 0xFFFFu) > n_bytes || ents[e].slot >= slots) {
                    cs_set_err("VARTEXT column %u: inconsistent dictionary entry", c);
                    return CSTRIPE_ERR;
                }
            std::vector<uint32_t> order(n_dict);
            for (uint32_t e = 0; e < n_dict; e++) order[e] = e;
            std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                return vt_cmp(gb + ents[a].boff, ents[a].ref & 0xFFFFu,
                              gb + ents[b].boff, ents[b].ref & 0xFFFFu) < 0;
            });
            cs_text_dict &d = s->text_dicts[c];
            d.offsets.assign(1, 0);
            d.bytes.clear();
            d.bytes.reserve(n_bytes);
            std::vector<uint32_t> s2r(slots, 0);
            for (uint32_t rk = 0; rk < n_dict; rk++) {
                const VtEntry &en = ents[order[rk]];
                const uint32_t len = (uint32_t)(en.ref & 0xFFFFu);
                d.bytes.insert(d.bytes.end(), gb + en.boff, gb + en.boff + len);
                d.offsets.push_back(d.bytes.size());
                s2r[en.slot] = rk;
            }
            HIP_TRY(vt.alloc(d_s2r, slots * sizeof(uint32_t)));
            HIP_TRY(hipMemcpyAsync(d_s2r, s2r.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, g->stream));
            HIP_TRY(hipEventRecord(vt.ev[5], g->stream));
            hipLaunchKernelGGL(vt_remap_kernel, dim3(ncks), dim3(AGG_BLOCK), 0, g->stream,
                               d_chunks + col_cbeg[ci], d_vslot, vbeg, d_s2r, g->d_scratch);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(vt.ev[6], g->stream));
            HIP_TRY(hipStreamSynchronize(g->stream));
            (void)hipEventElapsedTime(&ms, vt.ev[5], vt.ev[6]);
            s->last_text_remap_ms += ms;
            if (g->like_form[c] == CSTRIPE_LIKE_FORM_DICT) {
                int _rc = like_build(ci, d_ent, n_dict, slots, d_vslot);
                if (_rc != CSTRIPE_OK) return _rc;
            }
            vt.free_from(mark);
        }
    }

    /* ---- VARTEXT predicates -> integer atoms over ranks (cstripe.h) ---- */
    for (size_t i = 0; i < s->preds.size(); i++) {
        const cstripe_pred &q = s->preds[i];
        if (cs_col_type(s, q.column) != CSTRIPE_VARTEXT) continue;
        if (g->mpred_slot[i] >= 0) continue;   /* IN / NOT IN: sets_build */
        const cs_text_dict &d = s->text_dicts[q.column];
        const std::string &cst = s->text_consts[(size_t)q.ival];
        const int64_t n = (int64_t)d.offsets.size() - 1;
        auto count_below = [&](bool or_equal) -> int64_t {
            int64_t lo = 0, hi = n;
            while (lo < hi) {
                const int64_t mid = (lo + hi) / 2;
                const int cmp = vt_cmp(d.bytes.data() + d.offsets[mid],
                                       d.offsets[mid + 1] - d.offsets[mid],
                                       (const uint8_t *)cst.data(), cst.size());
                if (cmp < 0 || (or_equal && cmp == 0)) lo = mid + 1; else hi = mid;
            }
            return lo;
        };
        const int64_t lb = count_below(false), ub = count_below(true);
        uint8_t op = (uint8_t)q.op;
        int64_t iv = 0;
        switch (q.op) {
            case CSTRIPE_PRED_EQ:
            case CSTRIPE_PRED_NE: iv = lb != ub ? lb : -1; break;   /* -1: absent */
            case CSTRIPE_PRED_LT: iv = lb; break;
            case CSTRIPE_PRED_LE: op = CSTRIPE_PRED_LT; iv = ub; break;
            case CSTRIPE_PRED_GE: op = CSTRIPE_PRED_GT; iv = lb - 1; break;
            case CSTRIPE_PRED_GT: iv = ub - 1; break;
            default: cs_set_err("bad predicate op %u", q.op); return CSTRIPE_ERR_ARG;
        }
        g->tpred_op[i] = op;
        g->tpred_ival[i] = iv;
    }
    return CSTRIPE_OK;
}

/* =====================================================================
 * Value sets — IN / NOT IN and the device semi-join filter.
 *
 * No query kernel knows about sets. At stage each distinct (column, set)
 * pair is turned into a one-byte MEMBERSHIP column in scratch (a member
 * slot), so `x IN S` is the integer atom member == 1 and `x NOT IN S` is
 * member == 0 on every surface — the arrangement VARTEXT uses for ranks.
 *   build   set_build_kernel: the int64 set (uploaded host copy, VARTEXT
 *           ranks, or the caller's device array) into a bitmap over
 *           [lo, hi] (atomicOr on u32 words) or an open-addressing table
 *           (64-bit atomicCAS claims, multiplicative hash, linear probing;
 *           the EMPTY pattern is a legal key, kept in a flag word)
 *   probe   set_probe_kernel: walks each selected chunk's value stream by
 *           value index through col_value (raw, decoded-in-scratch and
 *           canonical chunks alike), tests the table — read-only by then —
 *           with plain loads, and stores four 0/1 bytes per lane
 * ===================================================================== */

#define SET_EMPTY      (~0ull)
#define SET_HASH_MUL   0x9E3779B97F4A7C15ull
#define SET_PROBE_VALS 4u                       /* values per lane */
#define SET_TILE       (AGG_BLOCK * SET_PROBE_VALS)

struct SetTable {
    const uint32_t *bits;                 /* bitmap form, else null */
    const unsigned long long *keys;       /* hash form */
    const uint32_t *has_empty;            /* hash form: SET_EMPTY is a member */
    int64_t lo, hi;                       /* bitmap range */
    uint64_t mask;                        /* hash: slots - 1 */
    uint32_t shift;                       /* hash: 64 - log2(slots) */
    uint32_t pad;
};

__device__ inline uint64_t set_slot(uint64_t key, uint32_t shift)
{
    return (key * SET_HASH_MUL) >> shift;
}

/* [min, max] of a device array: per-lane strided scan, wave shuffle reduce,
 * one atomic pair per wave on sign-flipped (order-preserving unsigned) words */
__global__ __launch_bounds__(AGG_BLOCK) void set_range_kernel(
    const int64_t *__restrict__ vals, uint64_t n, unsigned long long *out)
{
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * AGG_BLOCK) {
        const int64_t v = vals[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const int64_t a = __shfl_down(mn, off, WAVE), b = __shfl_down(mx, off, WAVE);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (threadIdx.x % WAVE == 0) {
        atomicMin(&out[0], (unsigned long long)mn ^ 0x8000000000000000ull);
        atomicMax(&out[1], (unsigned long long)mx ^ 0x8000000000000000ull);
    }
}

int csgpu_set_range(const int64_t *dev_vals, uint64_t n, int64_t *lo, int64_t *hi, int *dev_id)
{
    if (!cstripe_gpu_available()) { cs_set_err("scan_begin_sets: a device set needs a visible MI355X"); return CSTRIPE_ERR_NOGPU; }
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, dev_vals) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        cs_set_err("scan_begin_sets: on_device set values are not a device pointer");
        return CSTRIPE_ERR_ARG;
    }
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(at.device));
    *dev_id = at.device;
    unsigned long long *d_out = nullptr;
    unsigned long long h_out[2] = {~0ull, 0ull};
    int rc = CSTRIPE_OK;
    auto fail = [&](hipError_t e, const char *what) {
        if (e == hipSuccess || rc != CSTRIPE_OK) return;
        cs_set_err("scan_begin_sets: %s failed: %s", what, hipGetErrorString(e));
        rc = CSTRIPE_ERR;
    };
    fail(hipMalloc(&d_out, sizeof(h_out)), "hipMalloc");
    if (rc == CSTRIPE_OK) {
        fail(hipMemcpy(d_out, h_out, sizeof(h_out), hipMemcpyHostToDevice), "hipMemcpy");
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n + AGG_BLOCK - 1) / AGG_BLOCK, 1024);
        if (rc == CSTRIPE_OK) {
            hipLaunchKernelGGL(set_range_kernel, dim3(grid), dim3(AGG_BLOCK), 0, 0, dev_vals, n, d_out);
            fail(hipGetLastError(), "set_range_kernel");
            fail(hipMemcpy(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost), "hipMemcpy");
        }
        (void)hipFree(d_out);
    }
    (void)hipSetDevice(prev);
    if (rc != CSTRIPE_OK) return rc;
    *lo = (int64_t)(h_out[0] ^ 0x8000000000000000ull);
    *hi = (int64_t)(h_out[1] ^ 0x8000000000000000ull);
    return CSTRIPE_OK;
}

/* insert vals[0..n) into the table. bits != null: bitmap over [lo, hi] (a
 * value outside it — a device set that changed since begin — is dropped, the
 * index never leaves the allocation). Else hash: slots >= 2n, so a probe
 * sequence always meets its key or an EMPTY slot. */
__global__ __launch_bounds__(AGG_BLOCK) void set_build_kernel(
    const int64_t *__restrict__ vals, uint64_t n, uint32_t *bits,
    unsigned long long *keys, uint32_t *has_empty, SetTable t)
{
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * AGG_BLOCK) {
        const int64_t v = vals[i];
        if (bits) {
            if (v < t.lo || v > t.hi) continue;
            const uint64_t d = (uint64_t)v - (uint64_t)t.lo;
            atomicOr(&bits[d >> 5], 1u << (d & 31u));
            continue;
        }
        const unsigned long long key = (unsigned long long)v;
        if (key == SET_EMPTY) { atomicOr(has_empty, 1u); continue; }
        uint64_t h = set_slot(key, t.shift);
        for (uint64_t tries = 0; tries <= t.mask; tries++) {
            const unsigned long long prev = atomicCAS(&keys[h], SET_EMPTY, key);
            if (prev == SET_EMPTY || prev == key) break;
            h = (h + 1) & t.mask;
        }
    }
}

__device__ inline uint32_t set_test(const SetTable &t, int64_t v)
{
    if (t.bits) {
        if (v < t.lo || v > t.hi) return 0;
        const uint64_t d = (uint64_t)v - (uint64_t)t.lo;
        return (t.bits[d >> 5] >> (d & 31u)) & 1u;
    }
    const unsigned long long key = (unsigned long long)v;
    if (key == SET_EMPTY) return *t.has_empty & 1u;
    uint64_t h = set_slot(key, t.shift);
    for (uint64_t tries = 0; tries <= t.mask; tries++) {
        const unsigned long long k = t.keys[h];
        if (k == key) return 1;
        if (k == SET_EMPTY) return 0;
        h = (h + 1) & t.mask;
    }
    return 0;
}

/* one block per (chunk group, tile of SET_TILE values); lane: four
 * consecutive value indexes, one dword of 0/1 bytes. The member region is
 * padded to 16 bytes, so the tail dword stays inside it. */
__global__ __launch_bounds__(AGG_BLOCK) void set_probe_kernel(
    const uint8_t *__restrict__ data, uint8_t *scratch,
    const ColLoc *__restrict__ colloc, const uint32_t *__restrict__ n_present,
    uint32_t n_proj, uint32_t key_proj, uint32_t member_proj, uint32_t tiles_pg,
    SetTable t)
{
    const uint32_t gi = blockIdx.x / tiles_pg, tile = blockIdx.x % tiles_pg;
    const uint32_t np = n_present[gi];
    const uint32_t v0 = (tile * AGG_BLOCK + threadIdx.x) * SET_PROBE_VALS;
    if (v0 >= np) return;
    ColLoc key = colloc[(uint64_t)gi * n_proj + key_proj];
    key.flags |= 2;                       /* by value index: no exists bitmap */
    const uint64_t out_off = colloc[(uint64_t)gi * n_proj + member_proj].val_off;
    uint32_t word = 0;
    #pragma unroll
    for (uint32_t k = 0; k < SET_PROBE_VALS; k++) {
        if (v0 + k >= np) break;
        int64_t iv = 0;
        double fv = 0;
        col_value(data, scratch, nullptr, key, v0 + k, iv, fv);
        word |= set_test(t, iv) << (8u * k);
    }
    *(uint32_t *)(scratch + out_off + v0) = word;
}

static int sets_build(cstripe_scan *s, VtTemps &st)
{
    cs_gpu_state *g = s->gpu;
    cstripe_reader *r = s->r;
    const uint32_t n_proj = g->n_proj;
    int force = 0;                         /* CSTRIPE_SET_FORM_*, 0 = choose */
    if (const char *e = getenv("CSTRIPE_SET_FORM")) {
        if (!strcmp(e, "hash")) force = CSTRIPE_SET_FORM_HASH;
        else if (!strcmp(e, "bitmap")) force = CSTRIPE_SET_FORM_BITMAP;
    }
    for (hipEvent_t &e : st.ev) HIP_TRY(hipEventCreate(&e));

    /* the key columns must be readable: decode what lands in scratch, once.
     * Every query call decodes the same segments again (no decoded flag is
     * shared with them; redundant, harmless). The membership regions survive
     * those decodes because a decode kernel stores only inside its segment's
     * own 16-byte-padded region, never past it — what the VARTEXT rank
     * regions rely on too. */
    bool need_decode = false;
    for (const auto &ms : g->mslots)
        if (!ms.like && g->col_scratch[(size_t)g->proj_of_col[ms.col]]) need_decode = true;
    if (need_decode) {
        HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
        { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
        int h_err = 0;
        HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        if (h_err) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    }

    uint32_t tiles_pg = (g->max_group_rows + SET_TILE - 1) / SET_TILE;
    if (tiles_pg == 0) tiles_pg = 1;
    if ((uint64_t)g->n_groups * tiles_pg >= (1ull << 31)) { cs_set_err("gpu_stage: too many tiles for the set probe"); return CSTRIPE_ERR_ARG; }

    struct Built { bool ok = false; SetTable t{}; };
    std::vector<Built> per_set(s->sets.size());
    std::vector<uint32_t> h_np(g->n_groups);
    uint32_t *d_np = nullptr;
    HIP_TRY(st.alloc(d_np, (uint64_t)g->n_groups * sizeof(uint32_t)));
    float ms_f = 0;

    for (const auto &ms : g->mslots) {
        if (ms.like) continue;             /* filled by vartext_build */
        cs_value_set &vs = s->sets[ms.set];
        const bool vartext = r->cols[ms.col].type == CSTRIPE_VARTEXT;
        Built local;
        Built &b = vartext ? local : per_set[ms.set];   /* ranks are per column */
        if (!b.ok) {
            /* ---- the int64 entries and their range ---- */
            std::vector<int64_t> ranks;
            const std::vector<int64_t> *hv = &vs.vals;
            if (vartext) {
                const cs_text_dict &d = s->text_dicts[ms.col];
                const int64_t nd = (int64_t)d.offsets.size() - 1;
                for (const std::string &tx : vs.texts) {
                    int64_t lo = 0, hi = nd;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) / 2;
                        if (vt_cmp(d.bytes.data() + d.offsets[mid], d.offsets[mid + 1] - d.offsets[mid],
                                   (const uint8_t *)tx.data(), tx.size()) < 0) lo = mid + 1; else hi = mid;
                    }
                    if (lo < nd && vt_cmp(d.bytes.data() + d.offsets[lo], d.offsets[lo + 1] - d.offsets[lo],
                                          (const uint8_t *)tx.data(), tx.size()) == 0)
                        ranks.push_back(lo);
                }
                std::sort(ranks.begin(), ranks.end());
                ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
                hv = &ranks;
            }
            uint64_t n = vs.on_device ? vs.n : hv->size();
            int64_t lo = 0, hi = 0;
            if (n) {
                lo = vs.on_device ? vs.lo : hv->front();
                hi = vs.on_device ? vs.hi : hv->back();
            }
            if (vs.on_device && n && vs.dev_id != g->device) {
                cs_set_err("gpu_stage: set %u lives on device %d, the scan is staged on device %d",
                           ms.set, vs.dev_id, g->device);
                return CSTRIPE_ERR_ARG;
            }
            /* ---- form ---- */
            const uint64_t span = (uint64_t)hi - (uint64_t)lo;         /* hi - lo, exact */
            const bool bitmap_legal = span < (1ull << 32);
            const uint64_t want = std::max<uint64_t>(1ull << 16, 128 * n);
            int form = (bitmap_legal && span + 1 <= want) ? CSTRIPE_SET_FORM_BITMAP
                                                          : CSTRIPE_SET_FORM_HASH;
            if (force == CSTRIPE_SET_FORM_HASH) form = force;
            if (force == CSTRIPE_SET_FORM_BITMAP && bitmap_legal) form = force;
            /* ---- table ---- */
            const int64_t *d_vals = vs.on_device ? vs.dev_vals : nullptr;
            if (!vs.on_device && n) {
                int64_t *up = nullptr;
                HIP_TRY(st.alloc(up, n * sizeof(int64_t)));
                HIP_TRY(hipMemcpyAsync(up, hv->data(), n * sizeof(int64_t), hipMemcpyHostToDevice, g->stream));
                d_vals = up;
            }
            uint32_t *d_bits = nullptr, *d_flag = nullptr;
            unsigned long long *d_keys = nullptr;
            SetTable t{};
            t.lo = lo;
            t.hi = hi;
            uint64_t size;
            /* build time = clearing the table + the insert kernel (the host
             * set's upload above is not in it) */
            HIP_TRY(hipEventRecord(st.ev[0], g->stream));
            if (form == CSTRIPE_SET_FORM_BITMAP) {
                size = span + 1;
                const uint64_t words = (size + 31) / 32;
                void *q = nullptr;
                HIP_TRY(hipMalloc(&q, words * 4));
                g->set_bufs.push_back(q);
                d_bits = (uint32_t *)q;
                HIP_TRY(hipMemsetAsync(d_bits, 0, words * 4, g->stream));
            } else {
                uint64_t slots = 2;
                uint32_t lg = 1;
                while (slots < 2 * n) { slots <<= 1; lg++; }
                size = slots;
                void *q = nullptr;
                HIP_TRY(hipMalloc(&q, slots * 8 + 8));
                g->set_bufs.push_back(q);
                d_keys = (unsigned long long *)q;
                d_flag = (uint32_t *)(d_keys + slots);
                HIP_TRY(hipMemsetAsync(d_keys, 0xFF, slots * 8, g->stream));
                HIP_TRY(hipMemsetAsync(d_flag, 0, 8, g->stream));
                t.mask = slots - 1;
                t.shift = 64 - lg;
            }
            if (n) {
                const uint32_t grid = (uint32_t)std::min<uint64_t>((n + AGG_BLOCK - 1) / AGG_BLOCK, 4096);
                hipLaunchKernelGGL(set_build_kernel, dim3(grid), dim3(AGG_BLOCK), 0, g->stream,
                                   d_vals, n, d_bits, d_keys, d_flag, t);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(st.ev[1], g->stream));
            HIP_TRY(hipStreamSynchronize(g->stream));
            (void)hipEventElapsedTime(&ms_f, st.ev[0], st.ev[1]);
            s->last_set_build_ms += ms_f;
            t.bits = d_bits;
            t.keys = d_keys;
            t.has_empty = d_flag;
            b.t = t;
            b.ok = true;
            vs.form = form;
            vs.form_size = size;
        }
        /* ---- probe (an empty selection still reports the set's form) ---- */
        if (g->n_groups == 0) continue;
        for (uint32_t gi = 0; gi < g->n_groups; gi++) {
            const cs_selchunk &sc = s->sel[gi];
            h_np[gi] = r->stripes[sc.stripe].nodes[ms.col][sc.chunk].n.n_present;
        }
        HIP_TRY(hipMemcpyAsync(d_np, h_np.data(), h_np.size() * sizeof(uint32_t), hipMemcpyHostToDevice, g->stream));
        HIP_TRY(hipEventRecord(st.ev[2], g->stream));
        hipLaunchKernelGGL(set_probe_kernel, dim3(g->n_groups * tiles_pg), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_data, g->d_scratch, g->d_colloc, d_np, n_proj,
                           (uint32_t)g->proj_of_col[ms.col], ms.proj, tiles_pg, b.t);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(st.ev[3], g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));   /* h_np is reused */
        (void)hipEventElapsedTime(&ms_f, st.ev[2], st.ev[3]);
        s->last_set_probe_ms += ms_f;
    }
    return CSTRIPE_OK;
}

/* =====================================================================
 * Lookups — the device N:1 join with payload columns.
 *
 * No query kernel knows about lookups. At stage each payload of each lookup
 * becomes a DERIVED column: a sparse I64 column in scratch whose exists
 * bitmap, rank table and compacted values are all written here, so every
 * surface reads it through col_value like a table column with NULLs.
 *   build   lookup_build_kernel: key -> entry index, one table per lookup
 *           (its payloads share one probe). Direct form: a u32 entry array
 *           over [lo, hi] claimed by 32-bit atomicCAS. Hash form: the
 *           open-addressing table of the value sets (64-bit atomicCAS claims,
 *           set_slot, linear probing; key -1 is the EMPTY pattern and lives
 *           in a flag + entry word) plus a u32 entry word per slot, stored by
 *           the claim's winner. An insert that meets its own key already
 *           claimed raises the duplicate flag.
 *   probe   lookup_probe_kernel: one wave per 64-row word reads the key
 *           through col_value (NULL key: no match), looks it up with plain
 *           loads (the table is read-only by then), ballots the exists word
 *           and stores each row's entry index into a temporary u32 array
 *   rank    lookup_rank_kernel: one block per chunk group scans the words'
 *           popcounts into the rank table (present values before word w)
 *   gather  lookup_gather_kernel: each matched row stores payload[p][entry]
 *           at rank[w] + popc(below) for every payload
 * Wave width is 64 throughout; the ballot of a partial last word has its
 * unused high bits zero because lanes past the group's rows never match.
 * ===================================================================== */

#define LK_NONE 0xFFFFFFFFu
#define LK_WAVES (AGG_BLOCK / WAVE)
#define LK_BATCH_ROWS (1ull << 26)      /* rows per probe / gather batch */

struct LkTable {
    const unsigned long long *keys;   /* hash form: key words */
    const uint32_t *ents;             /* hash form: entry index per slot */
    const uint32_t *neg1;             /* hash form: [0] key -1 present, [1] its entry */
    const uint32_t *direct;           /* direct form, else null */
    int64_t lo, hi;                   /* direct range */
    uint64_t mask;                    /* hash: slots - 1 */
    uint32_t shift;                   /* hash: 64 - log2(slots) */
    uint32_t pad;
};

struct LkPayloads {
    const int64_t *src[CSTRIPE_MAX_LOOKUP_PAYLOADS];
    uint32_t proj[CSTRIPE_MAX_LOOKUP_PAYLOADS];
    uint32_t n;
    uint32_t pad;
};

/* insert keys[0..n) -> entry index. flag bit 0: a duplicate build key; bit 1:
 * a key outside the direct range (a device array that changed since begin;
 * the index never leaves the allocation). Hash: slots >= 2n, so a probe
 * sequence always meets its key or an EMPTY slot. */
__global__ __launch_bounds__(AGG_BLOCK) void lookup_build_kernel(
    const int64_t *__restrict__ keys, uint64_t n, unsigned long long *hkeys,
    uint32_t *hents, uint32_t *neg1, uint32_t *direct, uint32_t *flag, LkTable t)
{
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * AGG_BLOCK) {
        const int64_t v = keys[i];
        if (direct) {
            if (v < t.lo || v > t.hi) { atomicOr(flag, 2u); continue; }
            const uint64_t d = (uint64_t)v - (uint64_t)t.lo;
            if (atomicCAS(&direct[d], LK_NONE, (uint32_t)i) != LK_NONE) atomicOr(flag, 1u);
            continue;
        }
        const unsigned long long key = (unsigned long long)v;
        if (key == SET_EMPTY) {
            if (atomicCAS(&neg1[0], 0u, 1u) == 0u) neg1[1] = (uint32_t)i;
            else atomicOr(flag, 1u);
            continue;
        }
        uint64_t h = set_slot(key, t.shift);
        for (uint64_t tries = 0; tries <= t.mask; tries++) {
            const unsigned long long prev = atomicCAS(&hkeys[h], SET_EMPTY, key);
            if (prev == SET_EMPTY) { hents[h] = (uint32_t)i; break; }
            if (prev == key) { atomicOr(flag, 1u); break; }
            h = (h + 1) & t.mask;
        }
    }
}

__device__ inline uint32_t lookup_find(const LkTable &t, int64_t v)
{
    if (t.direct) {
        if (v < t.lo || v > t.hi) return LK_NONE;
        return t.direct[(uint64_t)v - (uint64_t)t.lo];
    }
    const unsigned long long key = (unsigned long long)v;
    if (key == SET_EMPTY) return t.neg1[0] ? t.neg1[1] : LK_NONE;
    uint64_t h = set_slot(key, t.shift);
    for (uint64_t tries = 0; tries <= t.mask; tries++) {
        const unsigned long long k = t.keys[h];
        if (k == key) return t.ents[h];
        if (k == SET_EMPTY) return LK_NONE;
        h = (h + 1) & t.mask;
    }
    return LK_NONE;
}

/* blocks_pg blocks per chunk group of the batch [g0, g0 + gridDim.x /
 * blocks_pg), one wave per 64-row word; ents holds the batch's rows, the
 * first of which is table-wide row ent_base. The exists
 * region of a derived column is (rows + 63) / 64 whole words (8-byte padded
 * at layout), so the word store stays inside it. */
__global__ __launch_bounds__(AGG_BLOCK) void lookup_probe_kernel(
    const uint8_t *data, const uint8_t *__restrict__ scratch,
    const uint32_t *__restrict__ rank, uint8_t *data_w,
    const GroupDesc *__restrict__ groups, const ColLoc *__restrict__ colloc,
    const uint64_t *__restrict__ rowbase, uint32_t *__restrict__ ents,
    uint32_t n_proj, uint32_t key_proj, uint32_t d_proj, uint32_t blocks_pg,
    uint32_t g0, uint64_t ent_base, LkTable t)
{
    const uint32_t gi = g0 + blockIdx.x / blocks_pg;
    const uint32_t w = (blockIdx.x % blocks_pg) * LK_WAVES + threadIdx.x / WAVE;
    const uint32_t rows = groups[gi].row_count;
    if ((uint64_t)w * WAVE >= rows) return;            /* wave-uniform */
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t row = w * WAVE + lane;
    uint32_t e = LK_NONE;
    if (row < rows) {
        const ColLoc key = colloc[(uint64_t)gi * n_proj + key_proj];
        int64_t iv = 0;
        double fv = 0;
        if (col_value(data, scratch, rank, key, row, iv, fv)) e = lookup_find(t, iv);
        ents[rowbase[gi] - ent_base + row] = e;
    }
    const uint64_t word = __ballot(e != LK_NONE);
    if (lane == 0)
        ((uint64_t *)(data_w + colloc[(uint64_t)gi * n_proj + d_proj].exists_off))[w] = word;
}

/* one block per chunk group: exclusive scan of the bitmap words' popcounts */
__global__ __launch_bounds__(AGG_BLOCK) void lookup_rank_kernel(
    const uint8_t *__restrict__ data, uint32_t *rank,
    const GroupDesc *__restrict__ groups, const ColLoc *__restrict__ colloc,
    uint32_t n_proj, uint32_t d_proj, uint32_t g0)
{
    __shared__ uint32_t wsum[LK_WAVES];
    const uint32_t gi = g0 + blockIdx.x;
    const uint32_t words = (groups[gi].row_count + 63) / 64;
    const ColLoc cl = colloc[(uint64_t)gi * n_proj + d_proj];
    const uint64_t *bm = (const uint64_t *)(data + cl.exists_off);
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    uint32_t base = 0;
    for (uint32_t w0 = 0; w0 < words; w0 += AGG_BLOCK) {
        const uint32_t w = w0 + threadIdx.x;
        const uint32_t c = w < words ? (uint32_t)__popcll(bm[w]) : 0u;
        uint32_t incl = c;
        for (uint32_t off = 1; off < WAVE; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, WAVE);
            if (lane >= off) incl += up;
        }
        if (lane == WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for (uint32_t k = 0; k < LK_WAVES; k++) {
            if (k < wave) pre += wsum[k];
            tot += wsum[k];
        }
        if (w < words) rank[cl.rank_off + w] = base + pre + incl - c;
        base += tot;
        __syncthreads();
    }
}

/* the probe's geometry; a matched row's value index is below the key's
 * n_present, which sized the value region */
__global__ __launch_bounds__(AGG_BLOCK) void lookup_gather_kernel(
    const uint8_t *__restrict__ data, uint8_t *scratch,
    const uint32_t *__restrict__ rank, const GroupDesc *__restrict__ groups,
    const ColLoc *__restrict__ colloc, const uint64_t *__restrict__ rowbase,
    const uint32_t *__restrict__ ents, uint32_t n_proj, uint32_t blocks_pg,
    uint32_t g0, uint64_t ent_base, LkPayloads pp)
{
    const uint32_t gi = g0 + blockIdx.x / blocks_pg;
    const uint32_t w = (blockIdx.x % blocks_pg) * LK_WAVES + threadIdx.x / WAVE;
    const uint32_t rows = groups[gi].row_count;
    if ((uint64_t)w * WAVE >= rows) return;
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t row = w * WAVE + lane;
    const ColLoc *cls = colloc + (uint64_t)gi * n_proj;
    const uint64_t word = ((const uint64_t *)(data + cls[pp.proj[0]].exists_off))[w];
    const uint64_t bit = 1ull << lane;
    if (!(word & bit)) return;
    const uint32_t idx = rank[cls[pp.proj[0]].rank_off + w] + (uint32_t)__popcll(word & (bit - 1));
    const uint32_t e = ents[rowbase[gi] - ent_base + row];
    #pragma unroll
    for (uint32_t p = 0; p < CSTRIPE_MAX_LOOKUP_PAYLOADS; p++)
        if (p < pp.n)
            ((int64_t *)(scratch + cls[pp.proj[p]].val_off))[idx] = pp.src[p][e];
}

/* temporaries of lookups_build: rowbase, entry indexes and the flag, plus
 * the uploaded keys and payloads of every host map */
static_assert(3 + CSTRIPE_MAX_LOOKUPS * (1 + CSTRIPE_MAX_LOOKUP_PAYLOADS) <=
                  sizeof(VtTemps::bufs) / sizeof(void *),
              "VtTemps::bufs is too small for the lookups' temporaries");

static int lookups_build(cstripe_scan *s, VtTemps &lt)
{
    cs_gpu_state *g = s->gpu;
    const uint32_t n_proj = g->n_proj;
    int force = 0;                         /* CSTRIPE_LOOKUP_FORM_*, 0 = choose */
    if (const char *e = getenv("CSTRIPE_LOOKUP_FORM")) {
        if (!strcmp(e, "hash")) force = CSTRIPE_LOOKUP_FORM_HASH;
        else if (!strcmp(e, "direct")) force = CSTRIPE_LOOKUP_FORM_DIRECT;
    }
    for (hipEvent_t &e : lt.ev) HIP_TRY(hipEventCreate(&e));

    /* the key columns must be readable: decode what lands in scratch (as
     * sets_build does; the derived regions survive later decodes for the
     * same reason the membership regions do) */
    bool need_decode = false;
    for (const cs_lookup &lk : s->lookups)
        if (g->col_scratch[(size_t)g->proj_of_col[lk.key_column]]) need_decode = true;
    if (need_decode && g->n_groups) {
        HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
        { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
        int h_err = 0;
        HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        if (h_err) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    }

    const uint32_t words_pg = (g->max_group_rows + 63) / 64;
    const uint32_t blocks_pg = words_pg ? (words_pg + LK_WAVES - 1) / LK_WAVES : 1;
    if ((uint64_t)g->n_groups * blocks_pg >= (1ull << 31)) { cs_set_err("gpu_stage: too many words for the lookup probe"); return CSTRIPE_ERR_ARG; }

    /* per-row entry indexes of one lookup and one batch of chunk groups at a
     * time: probe, rank scan and gather run batch by batch, so the temporary
     * stays at 4 B x LK_BATCH_ROWS (256 MB) however large the scan is.
     * CSTRIPE_LOOKUP_BATCH_ROWS (environment, read per stage) overrides the
     * batch size; a batch always holds at least one chunk group. */
    uint64_t batch_rows = LK_BATCH_ROWS;
    if (const char *e = getenv("CSTRIPE_LOOKUP_BATCH_ROWS")) {
        const long long v = atoll(e);
        if (v > 0) batch_rows = (uint64_t)v;
    }
    struct Batch { uint32_t g0, ng; uint64_t first_row; };
    std::vector<Batch> batches;
    std::vector<uint64_t> h_rowbase(g->n_groups);
    uint64_t total_rows = 0, max_batch = 0;
    for (uint32_t gi = 0; gi < g->n_groups; gi++) {
        const cs_selchunk &sc = s->sel[gi];
        const uint64_t rows = s->r->stripes[sc.stripe].group_rows[sc.chunk];
        h_rowbase[gi] = total_rows;
        if (batches.empty() ||
            total_rows + rows - batches.back().first_row > batch_rows)
            batches.push_back({gi, 0, total_rows});
        batches.back().ng++;
        total_rows += rows;
        max_batch = std::max(max_batch, total_rows - batches.back().first_row);
    }
    uint64_t *d_rowbase = nullptr;
    uint32_t *d_ents = nullptr, *d_flag = nullptr;
    HIP_TRY(lt.alloc(d_rowbase, (uint64_t)g->n_groups * sizeof(uint64_t)));
    HIP_TRY(lt.alloc(d_ents, max_batch * sizeof(uint32_t)));
    HIP_TRY(lt.alloc(d_flag, sizeof(uint32_t)));
    if (g->n_groups)
        HIP_TRY(hipMemcpyAsync(d_rowbase, h_rowbase.data(), h_rowbase.size() * sizeof(uint64_t),
                               hipMemcpyHostToDevice, g->stream));
    float ms_f = 0;

    for (size_t l = 0; l < s->lookups.size(); l++) {
        cs_lookup &lk = s->lookups[l];
        const uint64_t n = lk.n;
        if (lk.on_device && lk.dev_id != g->device) {
            cs_set_err("gpu_stage: lookup %u lives on device %d, the scan is staged on device %d",
                       (unsigned)l, lk.dev_id, g->device);
            return CSTRIPE_ERR_ARG;
        }
        const int64_t lo = n ? lk.klo : 0, hi = n ? lk.khi : 0;
        /* ---- form ---- */
        const uint64_t span = (uint64_t)hi - (uint64_t)lo;             /* hi - lo, exact */
        const bool direct_legal = span < 0xFFFFFFFFull;                /* range < 2^32 */
        const uint64_t want = std::max<uint64_t>(1ull << 16, 4 * n);
        int form = (direct_legal && span + 1 <= want) ? CSTRIPE_LOOKUP_FORM_DIRECT
                                                      : CSTRIPE_LOOKUP_FORM_HASH;
        if (force == CSTRIPE_LOOKUP_FORM_HASH) form = force;
        if (force == CSTRIPE_LOOKUP_FORM_DIRECT && direct_legal) form = force;
        /* ---- the build side on the device ---- */
        const int64_t *d_keys = lk.dev_keys;
        LkPayloads pp{};
        pp.n = lk.n_payloads;
        for (size_t ds = 0; ds < g->dslots.size(); ds++)
            if (g->dslots[ds].lookup == l) pp.proj[g->dslots[ds].payload] = g->dslots[ds].proj;
        for (uint32_t p = 0; p < lk.n_payloads; p++) pp.src[p] = lk.dev_payloads[p];
        if (!lk.on_device && n) {
            int64_t *up = nullptr;
            HIP_TRY(lt.alloc(up, n * sizeof(int64_t)));
            HIP_TRY(hipMemcpyAsync(up, lk.keys.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, g->stream));
            d_keys = up;
            for (uint32_t p = 0; p < lk.n_payloads; p++) {
                HIP_TRY(lt.alloc(up, n * sizeof(int64_t)));
                HIP_TRY(hipMemcpyAsync(up, lk.payloads[p].data(), n * sizeof(int64_t), hipMemcpyHostToDevice, g->stream));
                pp.src[p] = up;
            }
        }
        /* ---- table: build time = clearing it + the insert kernel ---- */
        unsigned long long *d_hkeys = nullptr;
        uint32_t *d_hents = nullptr, *d_neg1 = nullptr, *d_direct = nullptr;
        LkTable t{};
        t.lo = lo;
        t.hi = hi;
        uint64_t size;
        HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), g->stream));
        HIP_TRY(hipEventRecord(lt.ev[0], g->stream));
        if (form == CSTRIPE_LOOKUP_FORM_DIRECT) {
            size = span + 1;
            void *q = nullptr;
            HIP_TRY(hipMalloc(&q, size * 4));
            g->set_bufs.push_back(q);
            d_direct = (uint32_t *)q;
            HIP_TRY(hipMemsetAsync(d_direct, 0xFF, size * 4, g->stream));
        } else {
            uint64_t slots = 2;
            uint32_t lg = 1;
            while (slots < 2 * n) { slots <<= 1; lg++; }
            size = slots;
            void *q = nullptr;
            HIP_TRY(hipMalloc(&q, slots * 12 + 8));
            g->set_bufs.push_back(q);
            d_hkeys = (unsigned long long *)q;
            d_hents = (uint32_t *)(d_hkeys + slots);
            d_neg1 = d_hents + slots;
            HIP_TRY(hipMemsetAsync(d_hkeys, 0xFF, slots * 8, g->stream));
            HIP_TRY(hipMemsetAsync(d_neg1, 0, 8, g->stream));
            t.mask = slots - 1;
            t.shift = 64 - lg;
        }
        if (n) {
            const uint32_t grid = (uint32_t)std::min<uint64_t>((n + AGG_BLOCK - 1) / AGG_BLOCK, 4096);
            hipLaunchKernelGGL(lookup_build_kernel, dim3(grid), dim3(AGG_BLOCK), 0, g->stream,
                               d_keys, n, d_hkeys, d_hents, d_neg1, d_direct, d_flag, t);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(lt.ev[1], g->stream));
        uint32_t h_flag = 0;
        HIP_TRY(hipMemcpyAsync(&h_flag, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        (void)hipEventElapsedTime(&ms_f, lt.ev[0], lt.ev[1]);
        s->last_lookup_build_ms += ms_f;
        if (h_flag & 1u) {
            cs_set_err("gpu_stage: lookup %u: duplicate build keys in the device map "
                       "(build keys must be distinct)", (unsigned)l);
            return CSTRIPE_ERR_ARG;
        }
        if (h_flag & 2u) {
            cs_set_err("gpu_stage: lookup %u: a device build key lies outside the range found "
                       "at scan begin (the key array changed)", (unsigned)l);
            return CSTRIPE_ERR_ARG;
        }
        t.keys = d_hkeys;
        t.ents = d_hents;
        t.neg1 = d_neg1;
        t.direct = d_direct;
        lk.form = form;
        lk.form_size = size;
        /* ---- probe, rank scan, gather ---- */
        if (g->n_groups == 0) continue;
        HIP_TRY(hipEventRecord(lt.ev[2], g->stream));
        for (const Batch &b : batches) {
            /* one stream: a batch's gather is done with d_ents before the
             * next batch's probe overwrites it */
            const uint32_t grid = b.ng * blocks_pg;
            hipLaunchKernelGGL(lookup_probe_kernel, dim3(grid), dim3(AGG_BLOCK), 0, g->stream,
                               g->d_data, g->d_scratch, g->d_rank, g->d_data, g->d_groups, g->d_colloc,
                               d_rowbase, d_ents, n_proj, (uint32_t)g->proj_of_col[lk.key_column],
                               pp.proj[0], blocks_pg, b.g0, b.first_row, t);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(lookup_rank_kernel, dim3(b.ng), dim3(AGG_BLOCK), 0, g->stream,
                               g->d_data, g->d_rank, g->d_groups, g->d_colloc, n_proj, pp.proj[0], b.g0);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(lookup_gather_kernel, dim3(grid), dim3(AGG_BLOCK), 0, g->stream,
                               g->d_data, g->d_scratch, g->d_rank, g->d_groups, g->d_colloc,
                               d_rowbase, d_ents, n_proj, blocks_pg, b.g0, b.first_row, pp);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(lt.ev[3], g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        (void)hipEventElapsedTime(&ms_f, lt.ev[2], lt.ev[3]);
        s->last_lookup_probe_ms += ms_f;
    }
    return CSTRIPE_OK;
}

/* =====================================================================
 * Expressions — device-computed columns.
 *
 * No query kernel knows about expressions. At stage each expression becomes
 * a COMPUTED column: a sparse I64 column in scratch, laid out like a lookup's
 * derived column, whose exists bitmap, rank table and compacted values are
 * written by ONE kernel, expr_eval_kernel: one launch per expression, one
 * block per chunk group. The block walks its group in tiles of AGG_BLOCK
 * rows carrying a running base; each lane reads its row's inputs through
 * col_value (any stream shape), runs the postfix program, and the wave
 * ballots the non-NULL bit: lane 0 stores the exists word and the rank word
 * (running base + the waves before it, four wave totals through LDS), every
 * non-NULL lane its value at rank + popc(bits below). No per-row temporary,
 * no second pass. Lanes past the group's rows are NULL, so a partial last
 * word has zero high bits.
 *
 * The program travels by value in the kernel arguments and is wave-uniform:
 * the interpreter's switch does not diverge. The operand stack lives in LDS,
 * laid out [depth][thread] (a lane's entries sit AGG_BLOCK slots apart, so a
 * wave's access is one contiguous row: no bank conflicts), never in private
 * memory. Each entry is a value plus a flag byte: bit 0 NULL, bits 1..2 the
 * error code; the semantics are those of include/cstripe.h.
 * ===================================================================== */

#define EX_F_NULL  1u
#define EX_E_DIV0  1u       /* error codes, in flag bits 1..2 */
#define EX_E_RANGE 2u
#define EX_E_YEAR  3u

struct ExprProg {
    int64_t ival[CSTRIPE_MAX_EXPR_OPS];
    uint8_t op[CSTRIPE_MAX_EXPR_OPS];
    uint8_t proj[CSTRIPE_MAX_EXPR_OPS];   /* EX_COL: projected slot of the input */
    uint32_t n_ops;
    uint32_t pad;
};
static_assert(sizeof(ExprProg) <= 768, "the program travels in the kernel arguments");

/* per expression: range and count of the non-NULL results, and per error
 * kind the first row in scan order (group << 32 | row) whose final value
 * carries it, ~0 when none */
struct ExprState {
    long long mn, mx;
    unsigned long long cnt;
    unsigned long long err_row[3];
};

/* proleptic Gregorian (astronomical) year of a day count from 1970-01-01 */
__device__ inline int64_t expr_year(int64_t days)
{
    const int64_t z = days + 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int64_t doe = z - era * 146097;
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const int64_t mp = (5 * doy + 2) / 153;
    return yoe + era * 400 + (mp >= 10 ? 1 : 0);   /* January, February: next year of the March-based count */
}

/* writes only the computed column's own regions: the exists words
 * (rows + 63) / 64 (8-byte padded at layout), as many rank words, and value
 * indexes below the group's rows, which sized the value region */
__global__ __launch_bounds__(AGG_BLOCK) void expr_eval_kernel(
    uint8_t *data, uint8_t *scratch, uint32_t *rank,
    const GroupDesc *__restrict__ groups, const ColLoc *__restrict__ colloc,
    uint32_t n_proj, uint32_t e_proj, ExprState *state, ExprProg pg)
{
    __shared__ int64_t sv[CSTRIPE_MAX_EXPR_DEPTH][AGG_BLOCK];
    __shared__ uint8_t sf[CSTRIPE_MAX_EXPR_DEPTH][AGG_BLOCK];
    __shared__ uint32_t wsum[LK_WAVES];
    __shared__ long long rmn[LK_WAVES], rmx[LK_WAVES];
    __shared__ uint32_t rcnt[LK_WAVES];
    const uint32_t gi = blockIdx.x;
    const uint32_t rows = groups[gi].row_count;
    const ColLoc *cls = colloc + (uint64_t)gi * n_proj;
    uint64_t *bm = (uint64_t *)(data + cls[e_proj].exists_off);
    uint32_t *rk = rank + cls[e_proj].rank_off;
    int64_t *vals = (int64_t *)(scratch + cls[e_proj].val_off);
    const uint32_t t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    uint32_t base = 0, cnt = 0;
    long long mn = INT64_MAX, mx = INT64_MIN;
    for (uint32_t r0 = 0; r0 < rows; r0 += AGG_BLOCK) {
        const uint32_t row = r0 + t;
        const bool live = row < rows;
        uint32_t sp = 0;
        for (uint32_t i = 0; i < pg.n_ops; i++) {
            const uint32_t op = pg.op[i];
            int64_t v = 0;
            uint32_t f = 0;
            switch (op) {
                case CSTRIPE_EX_COL: {
                    double fv = 0;
                    f = EX_F_NULL;
                    if (live && col_value(data, scratch, rank, cls[pg.proj[i]], row, v, fv)) f = 0;
                    break;
                }
                case CSTRIPE_EX_CONST:
                    v = pg.ival[i];
                    break;
                case CSTRIPE_EX_NULL:
                    f = EX_F_NULL;
                    break;
                case CSTRIPE_EX_NEG: case CSTRIPE_EX_NOT: case CSTRIPE_EX_IS_NULL: case CSTRIPE_EX_YEAR: {
                    const int64_t a = sv[sp - 1][t];
                    const uint32_t fa = sf[sp - 1][t];
                    sp -= 1;
                    uint32_t err = fa >> 1;
                    if (op == CSTRIPE_EX_IS_NULL) {
                        v = fa & EX_F_NULL;
                    } else if (fa & EX_F_NULL) {
                        f = EX_F_NULL;
                    } else if (!err) {
                        if (op == CSTRIPE_EX_NOT) v = a == 0;
                        else if (op == CSTRIPE_EX_NEG) { if (__builtin_sub_overflow((int64_t)0, a, &v)) err = EX_E_RANGE; }
                        else if (a < -(1ll << 31) || a >= (1ll << 31)) err = EX_E_YEAR;
                        else v = expr_year(a);
                    }
                    f |= err << 1;
                    break;
                }
                case CSTRIPE_EX_AND: case CSTRIPE_EX_OR: {
                    /* Kleene, left to right: a clean left operand that decides
                     * (FALSE for AND, TRUE for OR) hides the right one */
                    const int64_t b = sv[sp - 1][t], a = sv[sp - 2][t];
                    const uint32_t fb = sf[sp - 1][t], fa = sf[sp - 2][t];
                    sp -= 2;
                    const int64_t decides = op == CSTRIPE_EX_AND ? 0 : 1;
                    if (fa >> 1) {
                        f = fa & ~EX_F_NULL;
                    } else if (!(fa & EX_F_NULL) && (a != 0) == decides) {
                        v = decides;
                    } else if (fb >> 1) {
                        f = fb & ~EX_F_NULL;
                    } else if (!(fb & EX_F_NULL) && (b != 0) == decides) {
                        v = decides;
                    } else if ((fa | fb) & EX_F_NULL) {
                        f = EX_F_NULL;
                    } else {
                        v = 1 - decides;
                    }
                    break;
                }
                case CSTRIPE_EX_COALESCE: {
                    const int64_t b = sv[sp - 1][t], a = sv[sp - 2][t];
                    const uint32_t fb = sf[sp - 1][t], fa = sf[sp - 2][t];
                    sp -= 2;
                    const bool take_a = (fa >> 1) || !(fa & EX_F_NULL);
                    v = take_a ? a : b;
                    f = take_a ? fa : fb;
                    break;
                }
                case CSTRIPE_EX_SELECT: {
                    const int64_t b = sv[sp - 1][t], a = sv[sp - 2][t], c = sv[sp - 3][t];
                    const uint32_t fb = sf[sp - 1][t], fa = sf[sp - 2][t], fc = sf[sp - 3][t];
                    sp -= 3;
                    if (fc >> 1) {
                        f = fc & ~EX_F_NULL;
                    } else {
                        const bool then = !(fc & EX_F_NULL) && c != 0;
                        v = then ? a : b;
                        f = then ? fa : fb;
                    }
                    break;
                }
                default: {
                    /* strict binary ops: the left operand's error, else the
                     * right one's, else NULL, else the op itself */
                    const int64_t b = sv[sp - 1][t], a = sv[sp - 2][t];
                    const uint32_t fb = sf[sp - 1][t], fa = sf[sp - 2][t];
                    sp -= 2;
                    uint32_t err = (fa >> 1) ? (fa >> 1) : (fb >> 1);
                    f = (fa | fb) & EX_F_NULL;
                    if (!f && !err) {
                        switch (op) {
                            case CSTRIPE_EX_ADD: if (__builtin_add_overflow(a, b, &v)) err = EX_E_RANGE; break;
                            case CSTRIPE_EX_SUB: if (__builtin_sub_overflow(a, b, &v)) err = EX_E_RANGE; break;
                            case CSTRIPE_EX_MUL: if (__builtin_mul_overflow(a, b, &v)) err = EX_E_RANGE; break;
                            case CSTRIPE_EX_DIV:
                                if (b == 0) err = EX_E_DIV0;
                                else if (b == -1) { if (__builtin_sub_overflow((int64_t)0, a, &v)) err = EX_E_RANGE; }
                                else v = a / b;
                                break;
                            case CSTRIPE_EX_MOD:
                                if (b == 0) err = EX_E_DIV0;
                                else if (b != -1) v = a % b;
                                break;
                            case CSTRIPE_EX_LT: v = a < b; break;
                            case CSTRIPE_EX_LE: v = a <= b; break;
                            case CSTRIPE_EX_GT: v = a > b; break;
                            case CSTRIPE_EX_GE: v = a >= b; break;
                            case CSTRIPE_EX_EQ: v = a == b; break;
                            default:            v = a != b; break;
                        }
                        if (err) v = 0;
                    }
                    f |= err << 1;
                    break;
                }
            }
            sv[sp][t] = v;
            sf[sp][t] = (uint8_t)f;
            sp++;
        }
        const int64_t v = sv[0][t];
        const uint32_t f = sf[0][t];
        if (live && (f >> 1))
            atomicMin(&state->err_row[(f >> 1) - 1], ((unsigned long long)gi << 32) | row);
        const bool present = live && f == 0;
        const uint64_t word = __ballot(present);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(word);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for (uint32_t k = 0; k < LK_WAVES; k++) {
            if (k < wave) pre += wsum[k];
            tot += wsum[k];
        }
        const uint32_t w = (r0 >> 6) + wave;
        if (lane == 0 && (uint64_t)w * WAVE < rows) {
            bm[w] = word;
            rk[w] = base + pre;
        }
        if (present) {
            vals[base + pre + (uint32_t)__popcll(word & ((1ull << lane) - 1))] = v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
            cnt++;
        }
        base += tot;
        __syncthreads();
    }
    /* range and count: wave reduce, then one atomic of each per block */
    for (uint32_t off = WAVE / 2; off; off >>= 1) {
        const long long omn = __shfl_xor(mn, off, WAVE), omx = __shfl_xor(mx, off, WAVE);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        cnt += __shfl_xor(cnt, off, WAVE);
    }
    if (lane == 0) { rmn[wave] = mn; rmx[wave] = mx; rcnt[wave] = cnt; }
    __syncthreads();
    if (t == 0) {
        for (uint32_t k = 1; k < LK_WAVES; k++) {
            mn = rmn[k] < mn ? rmn[k] : mn;
            mx = rmx[k] > mx ? rmx[k] : mx;
            cnt += rcnt[k];
        }
        if (cnt) {
            atomicMin(&state->mn, mn);
            atomicMax(&state->mx, mx);
            atomicAdd(&state->cnt, (unsigned long long)cnt);
        }
    }
}

static const char *const expr_err_text[3] = {"division by zero", "bigint out of range", "year out of range"};

static int exprs_build(cstripe_scan *s, VtTemps &et)
{
    cs_gpu_state *g = s->gpu;
    const uint32_t n_proj = g->n_proj;
    const size_t n_exprs = s->exprs.size();
    for (hipEvent_t &e : et.ev) HIP_TRY(hipEventCreate(&e));

    /* the input columns must be readable: decode what lands in scratch (as
     * lookups_build does; the computed regions survive later decodes for the
     * same reason the derived regions do) */
    bool need_decode = false;
    for (const cs_expr &ex : s->exprs)
        for (const cstripe_expr_op &op : ex.ops)
            if (op.op == CSTRIPE_EX_COL && g->col_scratch[(size_t)g->proj_of_col[op.column]]) need_decode = true;
    if (need_decode && g->n_groups) {
        HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
        { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
        int h_err = 0;
        HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        if (h_err) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    }

    std::vector<ExprState> h_state(n_exprs);
    for (ExprState &st : h_state) {
        st.mn = INT64_MAX;
        st.mx = INT64_MIN;
        st.cnt = 0;
        st.err_row[0] = st.err_row[1] = st.err_row[2] = ~0ull;
    }
    ExprState *d_state = nullptr;
    HIP_TRY(et.alloc(d_state, n_exprs * sizeof(ExprState)));
    HIP_TRY(hipMemcpyAsync(d_state, h_state.data(), n_exprs * sizeof(ExprState), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipEventRecord(et.ev[0], g->stream));
    for (size_t e = 0; e < n_exprs && g->n_groups; e++) {
        const cs_expr &ex = s->exprs[e];
        ExprProg pg{};
        pg.n_ops = (uint32_t)ex.ops.size();
        for (uint32_t i = 0; i < pg.n_ops; i++) {
            pg.op[i] = (uint8_t)ex.ops[i].op;
            pg.ival[i] = ex.ops[i].ival;
            if (ex.ops[i].op == CSTRIPE_EX_COL) pg.proj[i] = (uint8_t)g->proj_of_col[ex.ops[i].column];
        }
        hipLaunchKernelGGL(expr_eval_kernel, dim3(g->n_groups), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_data, g->d_scratch, g->d_rank, g->d_groups, g->d_colloc,
                           n_proj, g->eslots[e], d_state + e, pg);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(et.ev[1], g->stream));
    HIP_TRY(hipMemcpyAsync(h_state.data(), d_state, n_exprs * sizeof(ExprState), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    float ms_f = 0;
    (void)hipEventElapsedTime(&ms_f, et.ev[0], et.ev[1]);
    s->last_expr_ms = ms_f;
    for (size_t e = 0; e < n_exprs; e++) {
        /* like PG, the error of the first row in scan order that has one */
        const ExprState &st = h_state[e];
        int kind = -1;
        for (int k = 0; k < 3; k++)
            if (st.err_row[k] != ~0ull && (kind < 0 || st.err_row[k] < st.err_row[kind])) kind = k;
        if (kind >= 0) {
            cs_set_err("gpu_stage: expression %u: %s", (unsigned)e, expr_err_text[kind]);
            return CSTRIPE_ERR_ARG;
        }
    }
    for (size_t e = 0; e < n_exprs; e++) {
        cs_expr &ex = s->exprs[e];
        ex.n_present = h_state[e].cnt;
        ex.lo = ex.n_present ? h_state[e].mn : 0;
        ex.hi = ex.n_present ? h_state[e].mx : 0;
    }
    return CSTRIPE_OK;
}

/* true when the spec reads a VARTEXT column as a value: its ranks are a
 * per-scan coding, so only COUNT_COL (presence) means anything */
static bool agg_reads_vartext(const cstripe_reader *r, const cstripe_agg_spec &a)
{
    auto vt = [&](int32_t col) {
        return col >= 0 && col < (int32_t)r->head.column_count &&
               r->cols[col].type == CSTRIPE_VARTEXT;
    };
    switch (a.kind) {
        case CSTRIPE_AGG_COUNT_STAR:
        case CSTRIPE_AGG_COUNT_COL:        return false;
        case CSTRIPE_AGG_SUM_PROD_I64:
        case CSTRIPE_AGG_SUM_DISC_I64:     return vt(a.col_a) || vt(a.col_b);
        case CSTRIPE_AGG_SUM_DISC_TAX_I64: return vt(a.col_a) || vt(a.col_b) || vt(a.col_c);
        default:                           return vt(a.col_a);
    }
}

/* the one place a scan's predicates become device PredD atoms (scan_agg and
 * its grouped form, scan_agg_hashed, scan_select): a VARTEXT predicate goes
 * in as its stage-time translation over dictionary ranks */
static void fill_preds(const cstripe_scan *s, AggParams &p)
{
    const cs_gpu_state *g = s->gpu;
    p.n_preds = (uint32_t)s->preds.size();
    for (uint32_t i = 0; i < p.n_preds; i++) {
        const cstripe_pred &q = s->preds[i];
        p.preds[i].proj = (uint16_t)g->proj_of_col[q.column];
        p.preds[i].op = (uint8_t)q.op;
        uint8_t t = cs_col_type(s, q.column);
        p.preds[i].is_float = (t == CSTRIPE_F32 || t == CSTRIPE_F64) ? 1 : 0;
        p.preds[i].gend = (i + 1 == p.n_preds ||
                           s->preds[i + 1].or_group != q.or_group) ? 1 : 0;
        p.preds[i].ival = q.ival;
        p.preds[i].fval = q.fval;
        if (t == CSTRIPE_VARTEXT) {
            p.preds[i].op = g->tpred_op[i];
            p.preds[i].ival = g->tpred_ival[i];
            p.preds[i].fval = 0.0;
        }
        if (g->mpred_slot[i] >= 0) {
            /* IN / NOT IN, LIKE / NOT LIKE: one integer atom over the
             * membership column */
            p.preds[i].proj = (uint16_t)g->mslots[(size_t)g->mpred_slot[i]].proj;
            p.preds[i].op = CSTRIPE_PRED_EQ;
            p.preds[i].is_float = 0;
            p.preds[i].ival = (q.op == CSTRIPE_PRED_IN || q.op == CSTRIPE_PRED_LIKE) ? 1 : 0;
            p.preds[i].fval = 0.0;
        }
    }
}

/* projected slot of a table or derived column id — with cs_col_type the one
 * place that answers "type / slot of column id c" — -1 when out of range or
 * not projected */
/* true, with the error set, when `col` is a VARTEXT column staged in the
 * LIKE stream form: it was only pattern-matched and has no ranks to read */
static bool like_stream_refused(const cstripe_scan *s, int64_t col, const char *what)
{
    const cs_gpu_state *g = s->gpu;
    if (col < 0 || col >= (int64_t)g->like_form.size() ||
        g->like_form[(size_t)col] != CSTRIPE_LIKE_FORM_STREAM)
        return false;
    cs_set_err("%s: column %lld is only pattern-matched (LIKE stream form) and has no values to "
               "read — add it to cols_mask", what, (long long)col);
    return true;
}

static int proj_of(const cstripe_scan *s, int32_t col)
{
    if (col < 0 || col >= (int32_t)cs_scan_ncols(s)) return -1;
    return s->gpu->proj_of_col[col];
}

/* the AggParams header of scan_agg, its grouped form and scan_agg_hashed:
 * tile geometry, predicates and the aggregates' projected operand slots */
static int fill_agg_params(const cstripe_scan *s, const cstripe_agg_spec *aggs,
                           uint32_t n_aggs, AggParams &p)
{
    const cs_gpu_state *g = s->gpu;
    const cstripe_reader *r = s->r;
    p.n_aggs = n_aggs;
    p.n_proj = g->n_proj;
    p.tiles_per_group = (r->head.chunk_row_limit + TILE_ROWS - 1) / TILE_ROWS;
    if (p.tiles_per_group == 0) p.tiles_per_group = 1;
    p.n_groups = g->n_groups;
    fill_preds(s, p);
    for (uint32_t i = 0; i < n_aggs; i++) {
        p.aggs[i].kind = (uint8_t)aggs[i].kind;
        p.aggs[i].one = aggs[i].one;
        int pa = proj_of(s, aggs[i].col_a), pb = proj_of(s, aggs[i].col_b), pc = proj_of(s, aggs[i].col_c);
        if (aggs[i].kind != CSTRIPE_AGG_COUNT_STAR && like_stream_refused(s, aggs[i].col_a, "agg operand")) return CSTRIPE_ERR_ARG;
        if (aggs[i].kind != CSTRIPE_AGG_COUNT_STAR && pa < 0) { cs_set_err("agg %u: col_a not projected", i); return CSTRIPE_ERR_ARG; }
        if (agg_reads_vartext(r, aggs[i])) { cs_set_err("agg %u: a VARTEXT column can only be the operand of COUNT_COL", i); return CSTRIPE_ERR_ARG; }
        p.aggs[i].proj_a = (uint8_t)(pa < 0 ? 0 : pa);
        p.aggs[i].proj_b = (uint8_t)(pb < 0 ? 0 : pb);
        p.aggs[i].proj_c = (uint8_t)(pc < 0 ? 0 : pc);
    }
    return CSTRIPE_OK;
}

static bool aggs_all_integer(const cstripe_agg_spec *aggs, uint32_t n_aggs)
{
    for (uint32_t a = 0; a < n_aggs; a++)
        if (aggs[a].kind == CSTRIPE_AGG_SUM_F64 || aggs[a].kind == CSTRIPE_AGG_MIN_F64 ||
            aggs[a].kind == CSTRIPE_AGG_MAX_F64)
            return false;
    return true;
}

/* device accumulator cell -> wire partial: COUNT kinds are never NULL, every
 * other kind is NULL (value fields zero) iff no row contributed */
static cstripe_partial cell_to_partial(uint32_t kind, const AccCell &c)
{
    cstripe_partial o{};
    o.count = c.cnt;
    if (kind == CSTRIPE_AGG_COUNT_STAR || kind == CSTRIPE_AGG_COUNT_COL) {
        o.i128_lo = c.cnt;
        return o;
    }
    o.is_null = (c.cnt == 0) ? 1 : 0;
    if (o.is_null) return o;
    switch (kind) {
        case CSTRIPE_AGG_SUM_F64:
        case CSTRIPE_AGG_MIN_F64:
        case CSTRIPE_AGG_MAX_F64:
            o.f64 = c.f; break;
        case CSTRIPE_AGG_MIN_I64:
        case CSTRIPE_AGG_MAX_I64:
            o.i128_lo = c.lo; o.i128_hi = c.lo < 0 ? -1 : 0; break;
        default:
            o.i128_lo = c.lo; o.i128_hi = c.hi; break;
    }
    return o;
}

/* =====================================================================
 * scan_agg
 * ===================================================================== */

/* ev0..ev1 is the first stage (decode, or the fused kernel), ev1..ev2 the
 * aggregate; the stream must be synchronised past ev2 */
static void record_stage_ms(cstripe_scan *s)
{
    const cs_gpu_state *g = s->gpu;
    float ms_first = 0, ms_agg = 0;
    (void)hipEventElapsedTime(&ms_first, g->ev0, g->ev1);
    (void)hipEventElapsedTime(&ms_agg, g->ev1, g->ev2);
    s->last_decode_ms = ms_first;
    s->last_agg_ms = ms_agg;
    s->last_kernel_ms = ms_first + ms_agg;
}

/* ungrouped: d_final and the device flags -> out[n_aggs]; any flag is a
 * decode error here */
static int collect_ungrouped(cstripe_scan *s, const cstripe_agg_spec *aggs,
                             uint32_t n_aggs, cstripe_partial *out)
{
    cs_gpu_state *g = s->gpu;
    AccCell h_final[MAX_AGGS];
    int h_err = 0;
    HIP_TRY(hipMemcpyAsync(h_final, g->d_final, n_aggs * sizeof(AccCell), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (h_err) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    record_stage_ms(s);
    for (uint32_t a = 0; a < n_aggs; a++)
        out[a] = cell_to_partial(aggs[a].kind, h_final[a]);
    return CSTRIPE_OK;
}

/* waves per SIMD of multi_agg_kernel_ov = resident blocks per CU (a block is
 * one wave per SIMD); with the CU count this sizes its fixed grid */
#define OV_WAVES 4

/* resolve one scan_agg into the overlapped dense body's plan: the distinct
 * projected columns it touches (predicate slots first, each column once) and
 * the slot of every predicate and aggregate operand. false = not eligible,
 * the caller keeps the windowed body. */
static bool ov_build_plan(const cstripe_scan *s, const AggParams &p, OvPlan &pl)
{
    const cs_gpu_state *g = s->gpu;
    memset(&pl, 0, sizeof(pl));
    if (!g->all_dense || p.n_preds == 0 || p.n_preds > MAX_PREDS ||
        p.n_aggs == 0 || p.n_aggs > OV_MAX_AGGS || g->col_ov.size() != g->n_proj)
        return false;
    int slot_of[MAX_PROJ];
    for (int i = 0; i < MAX_PROJ; i++) slot_of[i] = -1;
    auto slot = [&](uint32_t proj) -> int {
        if (proj >= g->n_proj || !g->col_ov[proj]) return -1;
        if (slot_of[proj] < 0) {
            if (pl.n_slots == OV_MAX_SLOTS) return -1;
            pl.slot_proj[pl.n_slots] = (uint8_t)proj;
            slot_of[proj] = (int)pl.n_slots++;
        }
        return slot_of[proj];
    };
    for (uint32_t i = 0; i < p.n_preds; i++) {
        if (p.preds[i].is_float) return false;
        const int sl = slot(p.preds[i].proj);
        if (sl < 0) return false;
        pl.pred_ctl[i] = (uint32_t)sl | ((uint32_t)p.preds[i].op << 8) |
                         ((uint32_t)(p.preds[i].gend ? 1 : 0) << 16);
        pl.pred_val[i] = p.preds[i].ival;
        pl.sig |= ov_sig_pred(i, (uint32_t)sl);
    }
    pl.n_pslots = pl.n_slots;
    for (uint32_t a = 0; a < p.n_aggs; a++) {
        const AggD &ag = p.aggs[a];
        uint32_t n_ops;
        switch (ag.kind) {
            case CSTRIPE_AGG_COUNT_STAR:       n_ops = 0; break;
            case CSTRIPE_AGG_SUM_I64:
            case CSTRIPE_AGG_MIN_I64:
            case CSTRIPE_AGG_MAX_I64:          n_ops = 1; break;
            case CSTRIPE_AGG_SUM_PROD_I64:
            case CSTRIPE_AGG_SUM_DISC_I64:     n_ops = 2; break;
            case CSTRIPE_AGG_SUM_DISC_TAX_I64: n_ops = 3; break;
            default: return false;
        }
        const uint8_t ops[3] = {ag.proj_a, ag.proj_b, ag.proj_c};
        for (uint32_t k = 0; k < n_ops; k++) {
            const int sl = slot(ops[k]);
            if (sl < 0) return false;
            pl.agg_slot[a][k] = (uint8_t)sl;
            pl.sig |= ov_sig_op(a, k, (uint32_t)sl);
        }
        pl.ksig |= ov_ksig(a, ag.kind);
    }
    if (g->max_group_rows >= (1u << 28)) return false;   /* row * step stays u32 */
    /* work items at the finest tiling any instance uses */
    const uint64_t tiles = (g->max_group_rows + OV_R_ANY * AGG_BLOCK - 1) / (OV_R_ANY * AGG_BLOCK);
    if (g->n_groups == 0 || g->n_groups * (tiles ? tiles : 1) >= (1ull << 31)) return false;
    return true;
}

/* the plan's work items for an instance that takes R rows per lane */
static void ov_set_tiling(const cs_gpu_state *g, OvPlan &pl, uint32_t R)
{
    pl.tiles_pg = (g->max_group_rows + R * AGG_BLOCK - 1) / (R * AGG_BLOCK);
    if (pl.tiles_pg == 0) pl.tiles_pg = 1;
    pl.n_items = g->n_groups * pl.tiles_pg;
}

static int agg_ungrouped(cstripe_scan *s, const cstripe_agg_spec *aggs,
                         uint32_t n_aggs, const AggParams &p, cstripe_partial *out)
{
    cs_gpu_state *g = s->gpu;
    const uint32_t n_blocks = g->n_groups * p.tiles_per_group;
    if (n_blocks == 0) {
        /* empty selection — all-NULL partials (combine applies COUNT coalesce) */
        for (uint32_t a = 0; a < n_aggs; a++)
            out[a] = cell_to_partial(aggs[a].kind, AccCell{});
        s->last_kernel_ms = s->last_decode_ms = s->last_agg_ms = 0;
        s->last_agg_path = CSTRIPE_AGG_PATH_NONE;
        return CSTRIPE_OK;
    }

    HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
    HIP_TRY(hipEventRecord(g->ev0, g->stream));
    if (g->fusable && aggs_all_integer(aggs, n_aggs) && g->d_tiles) {
        /* fused decode+filter+aggregate: no scratch round trip; the first
         * stage time is the fused kernel (decode dominates) */
        s->last_fused = 1;
        s->last_agg_path = CSTRIPE_AGG_PATH_FUSED;
        auto launchf = [&](auto *kern) {
            hipLaunchKernelGGL(kern, dim3(g->n_tiles), dim3(AGG_BLOCK),
                               AGG_BLOCK * FUSE_STRIDE, g->stream,
                               g->d_data, g->d_segs, g->d_tiles, g->d_block,
                               g->d_error, p);
        };
        if (p.n_preds == 5 && n_aggs == 2) launchf(fused_agg_kernel<5, 2>);
        else if (p.n_preds == 5 && n_aggs == 4) launchf(fused_agg_kernel<5, 4>);
        else if (p.n_preds == 5 && n_aggs == 1) launchf(fused_agg_kernel<5, 1>);
        else if (p.n_preds == 1 && n_aggs == 1) launchf(fused_agg_kernel<1, 1>);
        else if (p.n_preds == 2 && n_aggs == 2) launchf(fused_agg_kernel<2, 2>);
        else launchf(fused_agg_kernel<-1, -1>);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(g->ev1, g->stream));
        { int _rc = launch_final_reduce(g, g->n_tiles, p); if (_rc != CSTRIPE_OK) return _rc; }
    } else {
        s->last_fused = 0;
        { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
        HIP_TRY(hipEventRecord(g->ev1, g->stream));
        OvPlan pl;
        if (ov_build_plan(s, p, pl)) {
            /* every referenced column is canonical P(L)/CONST everywhere:
             * overlapped body on a fixed, device-sized grid; each block
             * leaves one partial per aggregate */
            s->last_agg_path = CSTRIPE_AGG_PATH_DENSE_OV;
            uint32_t grid = 0;
            auto launcho = [&](auto *kern, uint32_t R) {
                ov_set_tiling(g, pl, R);
                grid = (uint32_t)g->n_cus * OV_WAVES;
                if (grid > pl.n_items) grid = pl.n_items;
                if (grid > g->max_blocks) grid = g->max_blocks;
                hipLaunchKernelGGL(kern, dim3(grid), dim3(AGG_BLOCK), 0, g->stream,
                                   g->d_data, g->d_groups, g->d_colloc, g->d_block,
                                   p, pl);
            };
            /* specialised shapes: TPC-H Q6 (two range predicates on one
             * column, two on a second, one on a third; sum(a*b) with b the
             * second column, count(*)) and count(*) under one predicate */
            constexpr uint64_t SIG_Q6 =
                ov_sig_pred(0, 0) | ov_sig_pred(1, 0) | ov_sig_pred(2, 1) |
                ov_sig_pred(3, 1) | ov_sig_pred(4, 2) |
                ov_sig_op(0, 0, 3) | ov_sig_op(0, 1, 1);
            constexpr uint32_t KSIG_Q6 = ov_ksig(0, CSTRIPE_AGG_SUM_PROD_I64) |
                                         ov_ksig(1, CSTRIPE_AGG_COUNT_STAR);
            constexpr uint32_t KSIG_CNT = ov_ksig(0, CSTRIPE_AGG_COUNT_STAR);
            const bool q6 = pl.n_slots == 4 && pl.n_pslots == 3 && p.n_preds == 5 &&
                            n_aggs == 2 && pl.sig == SIG_Q6 && pl.ksig == KSIG_Q6;
            const bool cnt = pl.n_slots == 1 && p.n_preds == 1 && n_aggs == 1 &&
                             pl.sig == 0 && pl.ksig == KSIG_CNT;
            auto launch_form = [&](auto win) {
                constexpr bool WIN = decltype(win)::value;
                if (q6)
                    launcho(multi_agg_kernel_ov<WIN, OV_R, 4, 3, 5, 2, true, OV_WAVES,
                                                SIG_Q6, KSIG_Q6>, OV_R);
                else if (cnt)
                    launcho(multi_agg_kernel_ov<WIN, OV_R, 1, 1, 1, 1, true, OV_WAVES,
                                                0, KSIG_CNT>, OV_R);
                else
                    launcho(multi_agg_kernel_ov<WIN, OV_R_ANY, OV_MAX_SLOTS, OV_MAX_SLOTS, 0,
                                                OV_MAX_AGGS, false, OV_WAVES>, OV_R_ANY);
            };
            /* zstd streams (rows 1..4 bytes apart) keep the window form */
            if (g->any_zr) launch_form(std::true_type{});
            else launch_form(std::false_type{});
            HIP_TRY(hipGetLastError());
            { int _rc = launch_final_reduce(g, grid, p); if (_rc != CSTRIPE_OK) return _rc; }
            HIP_TRY(hipEventRecord(g->ev2, g->stream));
            return collect_ungrouped(s, aggs, n_aggs, out);
        }
        s->last_agg_path = g->all_dense ? CSTRIPE_AGG_PATH_DENSE : CSTRIPE_AGG_PATH_GENERAL;
        if (g->all_dense) {
            /* all-dense: R-row windowed kernel (canonical closed-form or
             * decoded/raw typed arrays); hot shapes run R8 at a forced
             * 8 waves/SIMD, measured best */
            auto launchp = [&](auto *kern) {
                hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(AGG_BLOCK), 0, g->stream,
                                   g->d_data, g->d_scratch, g->d_groups,
                                   g->d_colloc, g->d_block, p);
            };
            if (p.n_preds == 5 && n_aggs == 2) launchp(multi_agg_kernel<5, 2, 8, 8>);
            else if (p.n_preds == 5 && n_aggs == 1) launchp(multi_agg_kernel<5, 1, 8, 8>);
            else if (p.n_preds == 1 && n_aggs == 1) launchp(multi_agg_kernel<1, 1, 8, 8>);
            else if (p.n_preds == 2 && n_aggs == 2) launchp(multi_agg_kernel<2, 2, 8, 8>);
            else if (p.n_preds == 5 && n_aggs == 4) launchp(multi_agg_kernel<5, 4, 8, 8>);
            else launchp(multi_agg_kernel<-1, -1, 4>);
        } else {
            auto launch = [&](auto *kern) {
                hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(AGG_BLOCK), 0, g->stream,
                                   g->d_data, g->d_scratch, g->d_rank, g->d_groups,
                                   g->d_colloc, g->d_block, p);
            };
            /* hot shapes compiled with unrolled pred/agg loops */
            if (p.n_preds == 5 && n_aggs == 2) launch(filter_agg_kernel<5, 2>);
            else if (p.n_preds == 5 && n_aggs == 1) launch(filter_agg_kernel<5, 1>);
            else if (p.n_preds == 1 && n_aggs == 1) launch(filter_agg_kernel<1, 1>);
            else if (p.n_preds == 2 && n_aggs == 2) launch(filter_agg_kernel<2, 2>);
            else launch(filter_agg_kernel<-1, -1>);
        }
        HIP_TRY(hipGetLastError());
        { int _rc = launch_final_reduce(g, n_blocks, p); if (_rc != CSTRIPE_OK) return _rc; }
    }
    HIP_TRY(hipEventRecord(g->ev2, g->stream));
    return collect_ungrouped(s, aggs, n_aggs, out);
}

/* grouped: merge the per-block tables just written (grouped_final_kernel),
 * close the timing window and read the device flags back */
static int grouped_merge(cs_gpu_state *g, const GroupParams &gp, uint32_t grid,
                         uint32_t per_block, int *h_err)
{
    hipLaunchKernelGGL(grouped_final_kernel, dim3(1), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_gkeys, g->d_gcells, grid, per_block,
                       g->d_gfkeys, g->d_gfcells, g->d_gn, g->d_error, gp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->ev2, g->stream));
    HIP_TRY(hipMemcpyAsync(h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return CSTRIPE_OK;
}

/* grouped: the merged keys, cells and count -> gr and out, sorted by key for
 * deterministic output (the oracle does the same) */
static int collect_grouped(cstripe_scan *s, const cstripe_agg_spec *aggs,
                           uint32_t n_aggs, cstripe_group_result *gr,
                           cstripe_partial *out)
{
    cs_gpu_state *g = s->gpu;
    uint32_t h_keys[CSTRIPE_MAX_GROUPS];
    std::vector<AccCell> h_cells((size_t)CSTRIPE_MAX_GROUPS * n_aggs);
    uint32_t h_n = 0;
    HIP_TRY(hipMemcpyAsync(h_keys, g->d_gfkeys, sizeof(h_keys), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(h_cells.data(), g->d_gfcells, h_cells.size() * sizeof(AccCell), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(&h_n, g->d_gn, 4, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    record_stage_ms(s);
    s->last_fused = 0;   /* every grouped path decodes to scratch */
    std::vector<uint32_t> order(h_n);
    for (uint32_t i = 0; i < h_n; i++) order[i] = i;
    std::sort(order.begin(), order.end(),
              [&](uint32_t a, uint32_t b) { return h_keys[a] < h_keys[b]; });
    gr->n_groups = h_n;
    for (uint32_t oi = 0; oi < h_n; oi++) {
        const uint32_t i = order[oi];
        gr->keys[oi] = h_keys[i];
        for (uint32_t a = 0; a < n_aggs; a++)
            out[(size_t)oi * n_aggs + a] =
                cell_to_partial(aggs[a].kind, h_cells[(size_t)i * n_aggs + a]);
    }
    return CSTRIPE_OK;
}

static int agg_grouped(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                       const uint32_t *group_cols, uint32_t n_group_cols,
                       const AggParams &p, cstripe_group_result *gr,
                       cstripe_partial *out)
{
    cs_gpu_state *g = s->gpu;
    const cstripe_reader *r = s->r;
    GroupParams gp{};
    gp.base = p;
    gp.n_group_cols = n_group_cols;
    for (uint32_t i = 0; i < n_group_cols; i++) {
        int pj = proj_of(s, (int32_t)group_cols[i]);
        if (pj < 0) { cs_set_err("group col %u not projected", group_cols[i]); return CSTRIPE_ERR_ARG; }
        if (cs_col_derived(s, group_cols[i])) { cs_set_err("group col %u is a derived (lookup) or computed (expression) column: scan_agg_grouped takes I8 or TEXT table columns; use scan_agg_hashed", group_cols[i]); return CSTRIPE_ERR_ARG; }
        if (r->cols[group_cols[i]].type != CSTRIPE_I8 &&
            r->cols[group_cols[i]].type != CSTRIPE_TEXT) { cs_set_err("group col %u must be I8 or TEXT", group_cols[i]); return CSTRIPE_ERR_ARG; }
        gp.gproj[i] = (uint32_t)pj;
    }
    gp.n_work = g->n_groups * p.tiles_per_group;
    if (gp.n_work == 0) {
        gr->n_groups = 0;
        s->last_kernel_ms = s->last_decode_ms = s->last_agg_ms = 0;
        return CSTRIPE_OK;
    }
    const uint32_t n_waves = AGG_BLOCK / WAVE;
    const uint32_t grid = gp.n_work < GRP_GRID ? gp.n_work : GRP_GRID;
    if (!g->d_gkeys) {
        HIP_TRY(hipMalloc(&g->d_gkeys, (uint64_t)GRP_GRID * n_waves * GRP_SLOTS * 4));
        HIP_TRY(hipMalloc(&g->d_gcells, (uint64_t)GRP_GRID * n_waves * GRP_SLOTS * MAX_AGGS * sizeof(AccCell)));
        HIP_TRY(hipMalloc(&g->d_gfkeys, CSTRIPE_MAX_GROUPS * 4));
        HIP_TRY(hipMalloc(&g->d_gfcells, (uint64_t)CSTRIPE_MAX_GROUPS * MAX_AGGS * sizeof(AccCell)));
        HIP_TRY(hipMalloc(&g->d_gn, 4));
    }
    int h_err = 0;

    if (g->all_dense) {
        /* multi-row grouped kernel (windowed loads + per-wave 16-slot LDS
         * tables); more than 16 distinct keys in a wave raise flag 8 */
        const uint32_t mlds = (n_waves * MGRP_SLOTS * n_aggs *
                               (uint32_t)sizeof(ThreadAcc) + 15u) & ~15u;
        bool need_decode = g->n_zsegs > 0;
        for (uint32_t pj = 0; pj < g->n_proj; pj++)
            if (g->col_scratch[pj]) need_decode = true;
        HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
        HIP_TRY(hipEventRecord(g->ev0, g->stream));
        if (need_decode) { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
        HIP_TRY(hipEventRecord(g->ev1, g->stream));
        auto launchmg = [&](auto *kern) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(AGG_BLOCK), mlds, g->stream,
                               g->d_data, g->d_scratch, g->d_groups, g->d_colloc,
                               g->d_gkeys, g->d_gcells, g->d_error, gp);
        };
        if (n_aggs == 5) launchmg(multi_grouped_kernel<5, 8>);
        else if (n_aggs == 1) launchmg(multi_grouped_kernel<1, 8>);
        else if (n_aggs == 2) launchmg(multi_grouped_kernel<2, 8>);
        else if (n_aggs == 4) launchmg(multi_grouped_kernel<4, 8>);
        else launchmg(multi_grouped_kernel<-1, 4>);
        HIP_TRY(hipGetLastError());
        { int _rc = grouped_merge(g, gp, grid, n_waves * MGRP_SLOTS, &h_err); if (_rc != CSTRIPE_OK) return _rc; }
        if (h_err & 4) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
        if (h_err == 0) return collect_grouped(s, aggs, n_aggs, gr, out);
        /* flag 8: fall through to the 64-group path */
    }

    /* any layout, up to CSTRIPE_MAX_GROUPS keys per wave */
    const uint32_t lds = n_waves * GRP_SLOTS * 4 + n_waves * GRP_SLOTS * n_aggs * (uint32_t)sizeof(ThreadAcc);
    HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
    HIP_TRY(hipEventRecord(g->ev0, g->stream));
    { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
    HIP_TRY(hipEventRecord(g->ev1, g->stream));
    auto launchg = [&](auto *kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(AGG_BLOCK), lds, g->stream,
                           g->d_data, g->d_scratch, g->d_rank, g->d_groups,
                           g->d_colloc, g->d_gkeys, g->d_gcells, g->d_error, gp);
    };
    if (n_aggs == 5) launchg(grouped_agg_kernel<5>);
    else if (n_aggs == 1) launchg(grouped_agg_kernel<1>);
    else if (n_aggs == 2) launchg(grouped_agg_kernel<2>);
    else launchg(grouped_agg_kernel<-1>);
    HIP_TRY(hipGetLastError());
    { int _rc = grouped_merge(g, gp, grid, n_waves * GRP_SLOTS, &h_err); if (_rc != CSTRIPE_OK) return _rc; }
    if (h_err & 4) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    if (h_err) { cs_set_err("too many distinct groups (device flag %d; caps: %d/wave, %d total)", h_err, GRP_SLOTS, CSTRIPE_MAX_GROUPS); return CSTRIPE_ERR; }
    return collect_grouped(s, aggs, n_aggs, gr, out);
}

int csgpu_agg(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
              const uint32_t *group_cols, uint32_t n_group_cols,
              cstripe_group_result *gr, cstripe_partial *out)
{
    if (!s->gpu) { cs_set_err("scan not staged — call cstripe_gpu_stage first (GPU required; no CPU fallback)"); return CSTRIPE_ERR_NOGPU; }
    if (n_aggs > MAX_AGGS) { cs_set_err("too many aggs"); return CSTRIPE_ERR_ARG; }
    if (s->preds.size() > MAX_PREDS) { cs_set_err("too many preds"); return CSTRIPE_ERR_ARG; }

    AggParams p{};
    { int _rc = fill_agg_params(s, aggs, n_aggs, p); if (_rc != CSTRIPE_OK) return _rc; }
    if (n_group_cols > 0)
        return agg_grouped(s, aggs, n_aggs, group_cols, n_group_cols, p, gr, out);
    return agg_ungrouped(s, aggs, n_aggs, p, out);
}

/* =====================================================================
 * next_batch — parity/fallback access: GPU-decode the next surviving chunk
 * group, copy decoded value streams back, expand to row-aligned on host
 * using the exists bitmap (ReadChunkGroupNextRow contract,
 * columnar_reader.c:868-901, batched).
 * ===================================================================== */

int csgpu_fetch_batch(cstripe_scan *s, uint32_t gi, cstripe_batch *batch)
{
    if (!s->gpu) { cs_set_err("scan not staged — call cstripe_gpu_stage first"); return CSTRIPE_ERR_NOGPU; }
    cs_gpu_state *g = s->gpu;
    cstripe_reader *r = s->r;
    if (gi >= s->sel.size()) return CSTRIPE_END;
    for (uint32_t c = 0; c < r->head.column_count && batch->col_values; c++)
        if (batch->col_values[c] && g->proj_of_col[c] >= 0 &&
            r->cols[c].type == CSTRIPE_VARTEXT) {
            cs_set_err("next_batch: column %u is VARTEXT — no batch access to variable-length "
                       "text; pass NULL for it (scan_select returns dictionary ranks)", c);
            return CSTRIPE_ERR_ARG;
        }

    /* make sure scratch holds decoded data (decode everything once) */
    if ((g->n_segs > 0 || g->n_zsegs > 0) && !g->batch_decoded) {
        HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
        { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
        int h_err = 0;
        HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        if (h_err) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
        g->batch_decoded = true;
    }

    const cs_selchunk &sc = s->sel[gi];
    const cs_stripe_info &st = r->stripes[sc.stripe];
    uint32_t rows = st.group_rows[sc.chunk];
    const uint8_t *stripe_base = r->stripe_base(st);

    std::vector<uint8_t> packed;
    for (uint32_t c = 0; c < r->head.column_count; c++) {
        int pj = g->proj_of_col[c];
        if (batch->col_values && batch->col_values[c] == nullptr) continue;
        if (pj < 0) continue;
        const cs_skipnode &nd = st.nodes[c][sc.chunk];
        uint32_t width = csf_type_width(r->cols[c].type);
        uint64_t soff = g->scratch_off[(uint64_t)gi * g->n_proj + pj];

        packed.resize(nd.n.decompressed_size);
        const ColLoc &cl = g->colloc_host[(uint64_t)gi * g->n_proj + pj];
        if (cl.flags & 4) {
            /* canonical chunk: closed-form device decode into the temp
             * buffer, then copy back (the agg path never materializes it) */
            if (g->tmp_bytes < nd.n.decompressed_size) {
                if (g->d_tmp) HIP_TRY(hipFree(g->d_tmp));
                g->tmp_bytes = align_up(nd.n.decompressed_size, 4096);
                HIP_TRY(hipMalloc(&g->d_tmp, g->tmp_bytes));
            }
            const uint32_t nv = (uint32_t)(nd.n.decompressed_size / width);
            const uint32_t grid2 = (nv + 255) / 256;
            hipLaunchKernelGGL(canon_decode_kernel, dim3(grid2), dim3(256), 0, g->stream,
                               g->d_data + cl.val_off, g->d_tmp, nv,
                               (uint32_t)cl.mode, (uint32_t)cl.L, width,
                               (uint64_t)cl.hval);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(packed.data(), g->d_tmp, nd.n.decompressed_size,
                                   hipMemcpyDeviceToHost, g->stream));
            HIP_TRY(hipStreamSynchronize(g->stream));
        } else if (soff != ~0ull) {  /* LZ4-decoded on device */
            HIP_TRY(hipMemcpyAsync(packed.data(), g->d_scratch + soff, nd.n.decompressed_size,
                                   hipMemcpyDeviceToHost, g->stream));
            HIP_TRY(hipStreamSynchronize(g->stream));
        } else {
            /* NONE / host-predecoded zstd: take staged raw from file side */
            if (nd.n.comp_type == CSTRIPE_COMP_NONE) {
                memcpy(packed.data(), stripe_base + nd.n.value_off, nd.n.decompressed_size);
            } else { /* zstd / pglz: decode host-side as at stage */
                for (const csf_seg &sg : st.nodes[c][sc.chunk].segs) {
                    if (nd.n.comp_type == CSTRIPE_COMP_ZSTD) {
                        size_t zr = ZSTD_decompress(packed.data() + sg.decomp_off, sg.decomp_len,
                                                    stripe_base + nd.n.value_off + sg.comp_off, sg.comp_len);
                        if (ZSTD_isError(zr) || zr != sg.decomp_len) { cs_set_err("zstd host decode failed"); return CSTRIPE_ERR_FORMAT; }
                    } else {
                        const uint8_t *pb = stripe_base + nd.n.value_off + sg.comp_off;
                        if (sg.comp_len < CSPGLZ_HDRSZ ||
                            cspglz_decompress(pb + CSPGLZ_HDRSZ,
                                              (int32_t)(sg.comp_len - CSPGLZ_HDRSZ),
                                              packed.data() + sg.decomp_off,
                                              (int32_t)sg.decomp_len) < 0) {
                            cs_set_err("pglz host decode failed");
                            return CSTRIPE_ERR_FORMAT;
                        }
                    }
                }
            }
        }

        /* expand packed -> row-aligned using the exists bitmap */
        uint8_t *dstv = (uint8_t *)batch->col_values[c];
        uint8_t *dstn = batch->col_nulls ? batch->col_nulls[c] : nullptr;
        const uint8_t *eb = stripe_base + nd.n.exists_off;
        uint32_t vidx = 0;
        if (nd.n.n_present == nd.n.row_count) {
            memcpy(dstv, packed.data(), (size_t)rows * width);
            if (dstn) memset(dstn, 0, rows);
        } else {
            for (uint32_t i = 0; i < rows; i++) {
                bool present = (eb[i / 8] >> (i % 8)) & 1;
                if (present) {
                    memcpy(dstv + (size_t)i * width, packed.data() + (size_t)vidx * width, width);
                    vidx++;
                } else {
                    memset(dstv + (size_t)i * width, 0, width);
                }
                if (dstn) dstn[i] = present ? 0 : 1;
            }
        }
    }

    batch->n_rows = rows;
    uint64_t first = st.meta.first_row_number;
    for (uint32_t k = 0; k < sc.chunk; k++) first += st.group_rows[k];
    batch->first_row_number = first;
    return CSTRIPE_OK;
}

int csgpu_next_batch(cstripe_scan *s, cstripe_batch *batch)
{
    int rc = csgpu_fetch_batch(s, (uint32_t)s->batch_pos, batch);
    if (rc == CSTRIPE_OK) s->batch_pos++;
    return rc;
}

/* =====================================================================
 * scan_select — device-side filtered row materialisation: the qual loop of
 * ColumnarScanNext (columnar_customscan.c:1854-1913: read a row, ExecQual,
 * return the rows that pass) with the rows themselves coming out, not an
 * aggregate of them. Deterministic three-kernel compaction, no global
 * atomics, same grid as the aggregate kernels (one block per chunk group x
 * TILE_ROWS tile, 4 waves of 64):
 *   select_mask_kernel    CNF per row -> __ballot pass word per 64-row
 *                         slice (1 bit/row) + one u32 count per tile
 *   select_offsets_kernel exclusive scan of the tile counts -> u64 bases,
 *                         grand total to one device word
 *   select_emit_kernel    rank inside the tile from the mask words, gather
 *                         the wanted columns through col_value, store value /
 *                         null byte / row number at base + rank
 * Output order is scan order (ascending row number) by construction.
 * ===================================================================== */

#define SEL_SLICES (TILE_ROWS / WAVE)      /* mask words per tile */
#define SEL_SCAN_ITEMS 8                   /* counts per thread per pass */
#define SEL_UNROLL 4                       /* mask slices in flight per wave */

struct SelCol {
    uint8_t *vals;          /* destination, physical width per row */
    uint8_t *nulls;         /* destination null bytes, or nullptr */
    uint32_t proj;
    uint32_t pad;
};

struct SelectParams {
    uint32_t n_cols, tiles_per_group;
    uint64_t *row_numbers;  /* destination, or nullptr */
    SelCol cols[MAX_PROJ];
};

/* A dense width-8 column chunk whose value j sits at a closed-form byte
 * position — raw or scratch-decoded typed arrays, canonical LIT / CONST /
 * P(L) for both codecs (the same positions col_value computes):
 *   value(j) = (load8(base + pos(j)) & keep) | high,
 *   pos(j)   = j == 0 ? p0 : j == 1 ? p1 : a * j + b
 * so the mask pass can issue its loads with no branch between them. */
struct SelFast {
    const uint8_t *base;
    uint64_t keep, high;
    uint32_t p0, p1, a, b;
    bool f64;
};

__device__ inline bool sel_fast_setup(const uint8_t *__restrict__ data,
                                      const uint8_t *__restrict__ scratch,
                                      const ColLoc &cl, SelFast &f)
{
    f.base = (cl.flags & 1) ? scratch + cl.val_off : data + cl.val_off;
    f.keep = ~0ull; f.high = 0;
    f.p0 = 0; f.p1 = 8; f.a = 8; f.b = 0;
    f.f64 = cl.type == CSTRIPE_F64;
    if (!(cl.flags & 2) || cl.width != 8) return false;
    if (!(cl.flags & 4)) return true;               /* typed array */
    const uint32_t L = cl.L;
    if (cl.mode == CSF_SEGMODE_LIT) {
        f.base += (uint64_t)cl.hval;                /* skip literal-run header */
        return true;
    }
    if (cl.mode == CSF_SEGMODE_CONST || cl.mode == CSF_SEGMODE_ZR_CONST) {
        f.keep = 0; f.high = (uint64_t)cl.hval;
        f.p1 = 0; f.a = 0;                          /* every row reads pos 0 */
        return true;
    }
    if (cl.mode > CSF_SEGMODE_P_BASE && cl.mode <= CSF_SEGMODE_P_BASE + 4) {
        f.p0 = 1; f.p1 = 9; f.a = L + 3; f.b = 6 - L;       /* canon_pos, lz4 */
    } else if (cl.mode > CSF_SEGMODE_ZRP_BASE && cl.mode <= CSF_SEGMODE_ZRP_BASE + 4) {
        f.p0 = 15; f.p1 = 23; f.a = L; f.b = 23 - L;        /* canon_pos, zstd */
    } else {
        return false;
    }
    if (L < 1 || L > 4) return false;
    f.keep = (~0ull) >> ((8u - L) * 8u);
    f.high = (uint64_t)cl.hval;
    return true;
}

template <int NPREDS>
__global__ __launch_bounds__(AGG_BLOCK) void select_mask_kernel(
    const uint8_t *__restrict__ data, const uint8_t *__restrict__ scratch,
    const uint32_t *__restrict__ rank, const GroupDesc *__restrict__ groups,
    const ColLoc *__restrict__ colloc, uint64_t *__restrict__ mask,
    uint32_t *__restrict__ counts, const AggParams params)
{
    const uint32_t n_preds = NPREDS >= 0 ? (uint32_t)NPREDS : params.n_preds;
    constexpr int UNROLL_PREDS = NPREDS > 0 ? NPREDS : 1;
    const uint32_t gid = blockIdx.x / params.tiles_per_group;
    const uint32_t tile = blockIdx.x % params.tiles_per_group;
    const GroupDesc g = groups[gid];
    const ColLoc *cols = colloc + g.colbase;
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;

    /* slices of this tile that hold rows; the rest of the 64 words are 0 */
    const uint32_t rc = g.row_count;
    const uint32_t t0 = tile * TILE_ROWS;
    const uint32_t n_sl = rc > t0 ? min((rc - t0 + WAVE - 1) / WAVE, (uint32_t)SEL_SLICES) : 0u;

    /* dense width-8 predicate columns in a closed-form layout (SelFast):
     * block-uniform, and only for the compile-time predicate counts */
    SelFast fast[UNROLL_PREDS];
    bool all_fast = NPREDS > 0;
    if (NPREDS > 0) {
        #pragma unroll
        for (int p = 0; p < UNROLL_PREDS; p++)
            all_fast = all_fast & sel_fast_setup(data, scratch,
                                                 cols[params.preds[p].proj], fast[p]);
    }

    uint32_t wcount = 0;
    /* each wave takes SEL_UNROLL consecutive slices per trip. Rows past
     * row_count are clamped to the chunk's last row and masked out, so no
     * load sits behind a per-row branch. */
    for (uint32_t sl0 = wid * SEL_UNROLL; sl0 < n_sl;
         sl0 += (AGG_BLOCK / WAVE) * SEL_UNROLL) {
        bool pass[SEL_UNROLL];
        if (all_fast) {
            /* one unaligned 8 B load per (slice, predicate), all issued
             * back to back before the first compare; predicates on the
             * same column re-load the same address (a cache hit) to keep
             * the sequence straight-line */
            uint64_t raw[SEL_UNROLL][UNROLL_PREDS];
            #pragma unroll
            for (uint32_t u = 0; u < SEL_UNROLL; u++) {
                const uint32_t rrow = min(t0 + (sl0 + u) * WAVE + lane, rc - 1);
                #pragma unroll
                for (int p = 0; p < UNROLL_PREDS; p++) {
                    const SelFast &f = fast[p];
                    const uint32_t pos = rrow < 2 ? (rrow == 0 ? f.p0 : f.p1)
                                                  : f.a * rrow + f.b;
                    __builtin_memcpy(&raw[u][p], f.base + pos, 8);
                }
            }
            #pragma unroll
            for (uint32_t u = 0; u < SEL_UNROLL; u++) {
                bool ps = t0 + (sl0 + u) * WAVE + lane < rc, gv = false;
                #pragma unroll
                for (int p = 0; p < UNROLL_PREDS; p++) {
                    const PredD &pr = params.preds[p];
                    const uint64_t r = (raw[u][p] & fast[p].keep) | fast[p].high;
                    const int64_t iv = (int64_t)r;
                    double fv;
                    if (fast[p].f64) __builtin_memcpy(&fv, &r, 8);
                    else fv = (double)iv;
                    gv = gv | pred_eval(pr, iv, fv);
                    if (pr.gend) { ps = ps & gv; gv = false; }
                }
                pass[u] = ps;
            }
        } else {
            #pragma unroll
            for (uint32_t u = 0; u < SEL_UNROLL; u++) {
                const uint32_t row = t0 + (sl0 + u) * WAVE + lane;
                const uint32_t rrow = min(row, rc - 1);  /* n_sl > 0 => rc >= 1 */
                bool ps = row < rc, gv = false;
                int last_proj = -1;
                int64_t liv = 0; double lfv = 0; bool lok = false;
                /* same OR-group fold as filter_agg_kernel */
                #pragma unroll UNROLL_PREDS
                for (uint32_t p = 0; p < n_preds; p++) {
                    const PredD &pr = params.preds[p];
                    if ((int)pr.proj != last_proj) {
                        lok = col_value(data, scratch, rank, cols[pr.proj], rrow, liv, lfv);
                        last_proj = (int)pr.proj;
                    }
                    gv = gv | (lok && pred_eval(pr, liv, lfv));
                    if (pr.gend) { ps = ps & gv; gv = false; }
                }
                pass[u] = ps;
            }
        }
        #pragma unroll
        for (uint32_t u = 0; u < SEL_UNROLL; u++) {
            const uint32_t sl = sl0 + u;
            if (sl >= n_sl) break;                      /* wave-uniform */
            const uint64_t word = __ballot(pass[u]);
            if (lane == 0) mask[(uint64_t)blockIdx.x * SEL_SLICES + sl] = word;
            wcount += (uint32_t)__popcll(word);
        }
    }
    for (uint32_t sl = n_sl + threadIdx.x; sl < SEL_SLICES; sl += AGG_BLOCK)
        mask[(uint64_t)blockIdx.x * SEL_SLICES + sl] = 0;

    __shared__ uint32_t lds[AGG_BLOCK / WAVE];
    if (lane == 0) lds[wid] = wcount;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < AGG_BLOCK / WAVE; w++) c += lds[w];
        counts[blockIdx.x] = c;
    }
}

/* one block: exclusive scan of n tile counts. Each pass covers
 * AGG_BLOCK * SEL_SCAN_ITEMS entries (thread-serial over its items, wave
 * shuffle scan, LDS across the 4 waves) with a u64 running carry. */
__global__ __launch_bounds__(AGG_BLOCK) void select_offsets_kernel(
    const uint32_t *__restrict__ counts, uint64_t *__restrict__ bases,
    uint64_t *__restrict__ total, uint32_t n)
{
    __shared__ uint32_t wsum[AGG_BLOCK / WAVE];
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    uint64_t carry = 0;
    for (uint64_t start = 0; start < n; start += AGG_BLOCK * SEL_SCAN_ITEMS) {
        const uint64_t i0 = start + (uint64_t)threadIdx.x * SEL_SCAN_ITEMS;
        uint32_t c[SEL_SCAN_ITEMS];
        uint32_t sum = 0;
        #pragma unroll
        for (uint32_t k = 0; k < SEL_SCAN_ITEMS; k++) {
            c[k] = i0 + k < n ? counts[i0 + k] : 0u;
            sum += c[k];
        }
        uint32_t inc = sum;
        #pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, WAVE);
            if ((int)lane >= d) inc += t;
        }
        if (lane == WAVE - 1) wsum[wid] = inc;
        __syncthreads();
        uint32_t wbase = 0, blk = 0;
        #pragma unroll
        for (uint32_t w = 0; w < AGG_BLOCK / WAVE; w++) {
            const uint32_t v = wsum[w];
            if (w < wid) wbase += v;
            blk += v;
        }
        uint64_t run = carry + wbase + (inc - sum);
        #pragma unroll
        for (uint32_t k = 0; k < SEL_SCAN_ITEMS; k++) {
            if (i0 + k < n) bases[i0 + k] = run;
            run += c[k];
        }
        carry += blk;
        __syncthreads();    /* wsum is rewritten by the next pass */
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(AGG_BLOCK) void select_emit_kernel(
    const uint8_t *__restrict__ data, const uint8_t *__restrict__ scratch,
    const uint32_t *__restrict__ rank, const GroupDesc *__restrict__ groups,
    const ColLoc *__restrict__ colloc, const uint64_t *__restrict__ mask,
    const uint64_t *__restrict__ bases, const uint64_t *__restrict__ rowbase,
    const SelectParams sp)
{
    __shared__ uint64_t s_word[SEL_SLICES];
    __shared__ uint32_t s_pre[SEL_SLICES];   /* passing rows in earlier slices */
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (wid == 0) {         /* SEL_SLICES == WAVE: one lane per mask word */
        const uint64_t w = mask[(uint64_t)blockIdx.x * SEL_SLICES + lane];
        const uint32_t pc = (uint32_t)__popcll(w);
        uint32_t inc = pc;
        #pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, WAVE);
            if ((int)lane >= d) inc += t;
        }
        s_word[lane] = w;
        s_pre[lane] = inc - pc;
    }
    __syncthreads();

    const uint32_t gid = blockIdx.x / sp.tiles_per_group;
    const uint32_t tile = blockIdx.x % sp.tiles_per_group;
    const ColLoc *cols = colloc + groups[gid].colbase;
    const uint64_t tile_base = bases[blockIdx.x];
    const uint64_t first_row = rowbase[gid];

    for (uint32_t sl = wid; sl < SEL_SLICES; sl += AGG_BLOCK / WAVE) {
        const uint64_t word = s_word[sl];
        if (word == 0) continue;                    /* wave-uniform skip */
        const uint64_t bit = 1ull << lane;
        if (!(word & bit)) continue;
        const uint32_t row = tile * TILE_ROWS + sl * WAVE + lane;
        const uint64_t idx = tile_base + s_pre[sl] +
                             (uint32_t)__popcll(word & (bit - 1));
        if (sp.row_numbers) sp.row_numbers[idx] = first_row + row;
        for (uint32_t c = 0; c < sp.n_cols; c++) {
            const SelCol &sc = sp.cols[c];
            const ColLoc &cl = cols[sc.proj];
            int64_t iv = 0; double fv = 0;
            const bool ok = col_value(data, scratch, rank, cl, row, iv, fv);
            if (!ok) { iv = 0; fv = 0; }            /* NULL slot: zero-filled */
            /* raw ABI representation at the physical width; idx*width keeps
             * every store naturally aligned */
            switch (cl.type) {
                case CSTRIPE_I8:  ((int8_t  *)sc.vals)[idx] = (int8_t)iv; break;
                case CSTRIPE_I16: ((int16_t *)sc.vals)[idx] = (int16_t)iv; break;
                case CSTRIPE_I32: ((int32_t *)sc.vals)[idx] = (int32_t)iv; break;
                case CSTRIPE_I64: ((int64_t *)sc.vals)[idx] = iv; break;
                case CSTRIPE_F32: ((float   *)sc.vals)[idx] = (float)fv; break;
                case CSTRIPE_TEXT: ((uint32_t *)sc.vals)[idx] = (uint32_t)iv; break;
                default:          ((double  *)sc.vals)[idx] = fv; break;
            }
            if (sc.nulls) sc.nulls[idx] = ok ? 0 : 1;
        }
    }
}

static int select_prepare(cstripe_scan *s, AggParams &p)
{
    cs_gpu_state *g = s->gpu;
    cstripe_reader *r = s->r;
    if (s->preds.size() > MAX_PREDS) { cs_set_err("too many preds"); return CSTRIPE_ERR_ARG; }
    p.n_preds = (uint32_t)s->preds.size();
    p.n_aggs = 0;
    p.n_proj = g->n_proj;
    p.tiles_per_group = (r->head.chunk_row_limit + TILE_ROWS - 1) / TILE_ROWS;
    if (p.tiles_per_group == 0) p.tiles_per_group = 1;
    p.n_groups = g->n_groups;
    fill_preds(s, p);
    for (hipEvent_t &e : g->sev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    const uint64_t n_tiles = (uint64_t)g->n_groups * p.tiles_per_group;
    if (n_tiles > 0 && !g->d_sel_mask) {
        HIP_TRY(hipMalloc(&g->d_sel_mask, n_tiles * SEL_SLICES * sizeof(uint64_t)));
        HIP_TRY(hipMalloc(&g->d_sel_counts, n_tiles * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&g->d_sel_bases, n_tiles * sizeof(uint64_t)));
        HIP_TRY(hipMalloc(&g->d_sel_total, sizeof(uint64_t)));
        /* table-wide row position of each surviving group's first row:
         * cumulative rows over ALL chunk groups in directory order, pruned
         * ones included — what cstripe_read_row counts on a predicate-free
         * scan (ColumnarReadNextRow's rowNumber, columnar_reader.c:322-361) */
        std::vector<uint64_t> h_rowbase(g->n_groups);
        uint64_t row_base = 0;
        size_t gi = 0;
        for (uint32_t si = 0; si < r->stripes.size(); si++) {
            const cs_stripe_info &st = r->stripes[si];
            for (uint32_t k = 0; k < st.meta.chunk_count; k++) {
                if (gi < s->sel.size() && s->sel[gi].stripe == si && s->sel[gi].chunk == k)
                    h_rowbase[gi++] = row_base;
                row_base += st.group_rows[k];
            }
        }
        if (gi != s->sel.size()) { cs_set_err("scan_select: selection not in directory order"); return CSTRIPE_ERR; }
        HIP_TRY(hipMalloc(&g->d_sel_rowbase, h_rowbase.size() * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(g->d_sel_rowbase, h_rowbase.data(),
                               h_rowbase.size() * sizeof(uint64_t),
                               hipMemcpyHostToDevice, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));   /* h_rowbase leaves scope */
    }
    return CSTRIPE_OK;
}

/* decode + mask + offsets on the scan's stream, then the one sync that
 * brings the total back. sev[0..3] bracket decode / mask / offsets. */
static int select_run_count(cstripe_scan *s, const AggParams &p)
{
    cs_gpu_state *g = s->gpu;
    const uint32_t n_tiles = g->n_groups * p.tiles_per_group;
    HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
    HIP_TRY(hipEventRecord(g->sev[0], g->stream));
    { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
    HIP_TRY(hipEventRecord(g->sev[1], g->stream));
    auto launchm = [&](auto *kern) {
        hipLaunchKernelGGL(kern, dim3(n_tiles), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_data, g->d_scratch, g->d_rank, g->d_groups,
                           g->d_colloc, g->d_sel_mask, g->d_sel_counts, p);
    };
    if (p.n_preds == 5) launchm(select_mask_kernel<5>);
    else if (p.n_preds == 1) launchm(select_mask_kernel<1>);
    else if (p.n_preds == 2) launchm(select_mask_kernel<2>);
    else launchm(select_mask_kernel<-1>);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->sev[2], g->stream));
    hipLaunchKernelGGL(select_offsets_kernel, dim3(1), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_sel_counts, g->d_sel_bases, g->d_sel_total, n_tiles);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->sev[3], g->stream));
    uint64_t h_total = 0;
    int h_err = 0;
    HIP_TRY(hipMemcpyAsync(&h_total, g->d_sel_total, sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (h_err) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    float ms_d = 0, ms_m = 0, ms_o = 0;
    (void)hipEventElapsedTime(&ms_d, g->sev[0], g->sev[1]);
    (void)hipEventElapsedTime(&ms_m, g->sev[1], g->sev[2]);
    (void)hipEventElapsedTime(&ms_o, g->sev[2], g->sev[3]);
    s->last_decode_ms = ms_d;
    s->last_select_mask_ms = ms_m;
    s->last_select_offsets_ms = ms_o;
    s->last_select_emit_ms = 0;
    s->last_agg_ms = 0;
    s->last_kernel_ms = ms_d + ms_m + ms_o;
    g->sel_total = h_total;
    g->sel_cached = true;
    return CSTRIPE_OK;
}

static void select_zero_timing(cstripe_scan *s)
{
    s->last_kernel_ms = s->last_decode_ms = s->last_agg_ms = 0;
    s->last_select_mask_ms = s->last_select_offsets_ms = s->last_select_emit_ms = 0;
}

int csgpu_select_count(cstripe_scan *s, uint64_t *n_rows)
{
    if (!s->gpu) { cs_set_err("scan not staged — call cstripe_gpu_stage first (GPU required; no CPU fallback)"); return CSTRIPE_ERR_NOGPU; }
    cs_gpu_state *g = s->gpu;
    AggParams p{};
    { int _rc = select_prepare(s, p); if (_rc != CSTRIPE_OK) return _rc; }
    if (g->n_groups == 0) {
        select_zero_timing(s);
        *n_rows = 0;
        return CSTRIPE_OK;
    }
    { int _rc = select_run_count(s, p); if (_rc != CSTRIPE_OK) return _rc; }
    *n_rows = g->sel_total;
    return CSTRIPE_OK;
}

int csgpu_select(cstripe_scan *s, cstripe_rows *out, uint64_t capacity,
                 int dst_on_device)
{
    if (!s->gpu) { cs_set_err("scan not staged — call cstripe_gpu_stage first (GPU required; no CPU fallback)"); return CSTRIPE_ERR_NOGPU; }
    cs_gpu_state *g = s->gpu;
    const uint32_t n_cols = cs_scan_ncols(s);

    SelectParams sp{};
    uint8_t widths[MAX_PROJ] = {0};
    uint32_t dst_col[MAX_PROJ] = {0};
    for (uint32_t c = 0; c < n_cols && out->col_values; c++) {
        if (!out->col_values[c]) continue;
        const int pj = proj_of(s, (int32_t)c);
        if (like_stream_refused(s, c, "scan_select")) return CSTRIPE_ERR_ARG;
        if (pj < 0) { cs_set_err("scan_select: column %u not projected", c); return CSTRIPE_ERR_ARG; }
        widths[sp.n_cols] = (uint8_t)csf_type_width(cs_col_type(s, c));
        dst_col[sp.n_cols] = c;
        sp.cols[sp.n_cols].proj = (uint32_t)pj;
        sp.n_cols++;
    }

    AggParams p{};
    { int _rc = select_prepare(s, p); if (_rc != CSTRIPE_OK) return _rc; }
    sp.tiles_per_group = p.tiles_per_group;
    if (g->n_groups == 0) {
        select_zero_timing(s);
        out->n_rows = 0;
        return CSTRIPE_OK;
    }

    float ms_d = 0, ms_m = 0, ms_o = 0;
    if (!g->sel_cached) {
        { int _rc = select_run_count(s, p); if (_rc != CSTRIPE_OK) return _rc; }
        ms_d = (float)s->last_decode_ms;
        ms_m = (float)s->last_select_mask_ms;
        ms_o = (float)s->last_select_offsets_ms;
    }
    const uint64_t n = g->sel_total;
    if (capacity < n) {
        cs_set_err("scan_select: capacity %llu < %llu selected rows",
                   (unsigned long long)capacity, (unsigned long long)n);
        return CSTRIPE_ERR_ARG;
    }
    if (n == 0) {
        s->last_decode_ms = ms_d;
        s->last_select_mask_ms = ms_m;
        s->last_select_offsets_ms = ms_o;
        s->last_select_emit_ms = 0;
        s->last_agg_ms = 0;
        s->last_kernel_ms = ms_d + ms_m + ms_o;
        out->n_rows = 0;
        return CSTRIPE_OK;
    }

    /* destinations: the caller's device pointers, or slices of the owned
     * compaction buffer (sized by the count) copied back per stream */
    uint64_t off_vals[MAX_PROJ], off_nulls[MAX_PROJ], off_rn = 0;
    if (dst_on_device) {
        for (uint32_t i = 0; i < sp.n_cols; i++) {
            sp.cols[i].vals = (uint8_t *)out->col_values[dst_col[i]];
            sp.cols[i].nulls = out->col_nulls ? out->col_nulls[dst_col[i]] : nullptr;
        }
        sp.row_numbers = out->row_numbers;
    } else {
        uint64_t need = 0;
        for (uint32_t i = 0; i < sp.n_cols; i++) {
            off_vals[i] = need;
            need = align_up(need + n * widths[i], 16);
            off_nulls[i] = need;
            if (out->col_nulls && out->col_nulls[dst_col[i]])
                need = align_up(need + n, 16);
        }
        off_rn = need;
        if (out->row_numbers) need += n * sizeof(uint64_t);
        if (need > g->sel_out_bytes) {
            if (g->d_sel_out) HIP_TRY(hipFree(g->d_sel_out));
            g->d_sel_out = nullptr;
            g->sel_out_bytes = 0;
            HIP_TRY(hipMalloc(&g->d_sel_out, need));
            g->sel_out_bytes = need;
        }
        for (uint32_t i = 0; i < sp.n_cols; i++) {
            sp.cols[i].vals = g->d_sel_out + off_vals[i];
            sp.cols[i].nulls = (out->col_nulls && out->col_nulls[dst_col[i]])
                                   ? g->d_sel_out + off_nulls[i] : nullptr;
        }
        sp.row_numbers = out->row_numbers ? (uint64_t *)(g->d_sel_out + off_rn) : nullptr;
    }

    const uint32_t n_tiles = g->n_groups * p.tiles_per_group;
    HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
    HIP_TRY(hipEventRecord(g->sev[0], g->stream));
    /* the emit pass gathers from decoded streams; decode re-runs per call
     * like scan_agg, so the timing means the same thing */
    { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
    HIP_TRY(hipEventRecord(g->sev[1], g->stream));
    hipLaunchKernelGGL(select_emit_kernel, dim3(n_tiles), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_data, g->d_scratch, g->d_rank, g->d_groups, g->d_colloc,
                       g->d_sel_mask, g->d_sel_bases, g->d_sel_rowbase, sp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->sev[2], g->stream));
    int h_err = 0;
    HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (h_err) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    if (!dst_on_device) {
        for (uint32_t i = 0; i < sp.n_cols; i++) {
            HIP_TRY(hipMemcpyAsync(out->col_values[dst_col[i]], sp.cols[i].vals,
                                   n * widths[i], hipMemcpyDeviceToHost, g->stream));
            if (sp.cols[i].nulls)
                HIP_TRY(hipMemcpyAsync(out->col_nulls[dst_col[i]], sp.cols[i].nulls,
                                       n, hipMemcpyDeviceToHost, g->stream));
        }
        if (sp.row_numbers)
            HIP_TRY(hipMemcpyAsync(out->row_numbers, sp.row_numbers,
                                   n * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
    }
    float ms_d2 = 0, ms_e = 0;
    (void)hipEventElapsedTime(&ms_d2, g->sev[0], g->sev[1]);
    (void)hipEventElapsedTime(&ms_e, g->sev[1], g->sev[2]);
    s->last_decode_ms = ms_d + ms_d2;
    s->last_select_mask_ms = ms_m;
    s->last_select_offsets_ms = ms_o;
    s->last_select_emit_ms = ms_e;
    s->last_agg_ms = 0;
    s->last_kernel_ms = ms_d + ms_d2 + ms_m + ms_o + ms_e;
    out->n_rows = n;
    return CSTRIPE_OK;
}

/* =====================================================================
 * Hashed GROUP BY (cstripe_scan_agg_hashed): the worker HashAggregate of
 * the reference's grouped plan (multi_explain.out:80-82,
 * multi_logical_optimizer.c:1807-1885) with no bound on the group count
 * but the caller's capacity. Three kernels on the scan's stream:
 *
 *   hash_init_kernel     key words = EMPTY, cells = acc_init identities.
 *                        Every call: a repeated call must not add onto the
 *                        previous call's sums.
 *   hash_agg_kernel      grid-stride blocks over (chunk group x 4096-row
 *                        tile), predicates exactly as grouped_agg_kernel.
 *                        The key tuple packs into ONE 64-bit word (host
 *                        picks per-column [lo, hi] from the selected
 *                        chunks' skip nodes), so claiming a slot is a single
 *                        8-byte CAS. Rows fold into a per-block LDS table
 *                        first (bounded probes; a row that finds no LDS
 *                        slot goes straight to the global table) — without
 *                        it a low-cardinality query funnels every row into
 *                        a few global words, and device atomics on one word
 *                        serialise. After its last tile the block flushes
 *                        its occupied LDS slots into the global table.
 *   hash_compact_kernel  appends the occupied global slots to dense arrays
 *                        through one device counter (wave-aggregated add);
 *                        the host sorts, so append order is free.
 *
 * No flag, fence, publish or spin-wait exists: every global word another
 * block may touch during hash_agg_kernel is updated only by device-scope
 * atomic read-modify-writes (CAS / add / min / max), and everything else is
 * visible at the kernel boundaries on the stream. The only plain loads of
 * such words are the first guess of the f64 min/max CAS loops: a stale
 * guess is an OLDER value of a monotonic word, so "my value does not
 * improve on it" still holds for the current value, and any other outcome
 * is re-checked by the CAS itself.
 * Every probe loop is bounded (LDS: HASH_LDS_PROBES; global: `slots`).
 * ===================================================================== */

#define HASH_EMPTY      (~0ull)
#define HASH_NONE       (~0ull)
#define HASH_LDS_PROBES 8
#define HASH_LDS_BUDGET (64u * 1024u)   /* bytes/block: two blocks fit a CU */
#define HASH_GRID       1024
#define HASH_ERR_RANGE  32              /* key outside its skip-node range */
#define HASH_ERR_FULL   64              /* global table full */
#define HASH_ERR_TEXT   128             /* order-key packed TEXT slot not canonical */

struct HashParams {
    AggParams base;
    uint32_t n_key_cols;
    uint32_t n_work;                    /* n_groups * tiles_per_group */
    uint32_t lds_slots;                 /* 0 = no LDS table, else power of 2 */
    uint32_t pad;
    uint32_t kproj[CSTRIPE_MAX_HASH_KEY_COLS];
    uint32_t kshift[CSTRIPE_MAX_HASH_KEY_COLS];
    int64_t  klo[CSTRIPE_MAX_HASH_KEY_COLS];
    uint64_t kspan[CSTRIPE_MAX_HASH_KEY_COLS];   /* hi - lo, unsigned */
    uint32_t klex[CSTRIPE_MAX_HASH_KEY_COLS];    /* TEXT packed by order key */
    uint64_t slots;                     /* global table, power of 2 */
};

/* a TEXT slot's C-collation order key (csf_text_lex_key, format.h) and its
 * inverse: the key is injective over canonical short-varlena slots (header
 * = payload length, zero padding, no NUL in the payload), which is what
 * lets a TEXT key column pack into its skip nodes' [min, max] */
__host__ __device__ inline uint32_t hash_text_lex(uint32_t slot)
{
    return (((slot >> 8) & 0xFFu) << 16) | (((slot >> 16) & 0xFFu) << 8) |
           ((slot >> 24) & 0xFFu);
}

__host__ __device__ inline uint32_t hash_text_slot(uint32_t lex)
{
    const uint32_t b1 = (lex >> 16) & 0xFFu, b2 = (lex >> 8) & 0xFFu, b3 = lex & 0xFFu;
    const uint32_t len = b3 ? 3u : (b2 ? 2u : (b1 ? 1u : 0u));
    return (((len + 1u) << 1) | 1u) | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

__device__ inline uint64_t hash_mix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

/* claim-or-find the key's slot in the global table: linear probing, one
 * 8-byte CAS per probe, at most `slots` probes; a full table sets
 * HASH_ERR_FULL and the caller drops the contribution (the host then fails
 * the whole call) */
__device__ inline uint64_t hash_global_insert(unsigned long long *gkeys, uint64_t slots,
                                              uint64_t h, uint64_t key, int *err)
{
    const uint64_t mask = slots - 1;
    uint64_t slot = h & mask;
    for (uint64_t n = 0; n < slots; n++) {
        const unsigned long long prev = atomicCAS(&gkeys[slot], HASH_EMPTY, key);
        if (prev == HASH_EMPTY || prev == key) return slot;
        slot = (slot + 1) & mask;
    }
    atomicOr(err, HASH_ERR_FULL);
    return HASH_NONE;
}

__global__ __launch_bounds__(AGG_BLOCK) void hash_init_kernel(
    unsigned long long *__restrict__ gkeys, ThreadAcc *__restrict__ gcells,
    unsigned long long *__restrict__ count, const HashParams hp)
{
    const uint32_t n_aggs = hp.base.n_aggs;
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; i < hp.slots;
         i += (uint64_t)gridDim.x * AGG_BLOCK) {
        gkeys[i] = HASH_EMPTY;
        for (uint32_t a = 0; a < n_aggs; a++) {
            ThreadAcc z;
            acc_init(z, hp.base.aggs[a].kind);
            gcells[i * n_aggs + a] = z;
        }
    }
}

template <int NAGGS>
__global__ __launch_bounds__(AGG_BLOCK) void hash_agg_kernel(
    const uint8_t *__restrict__ data, const uint8_t *__restrict__ scratch,
    const uint32_t *__restrict__ rank, const GroupDesc *__restrict__ groups,
    const ColLoc *__restrict__ colloc, unsigned long long *gkeys,
    ThreadAcc *gcells, int *err, const HashParams hp)
{
    const AggParams &params = hp.base;
    const uint32_t n_aggs_ct = NAGGS >= 0 ? (uint32_t)NAGGS : params.n_aggs;
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t n_waves = AGG_BLOCK / WAVE;
    const uint32_t L = hp.lds_slots;

    extern __shared__ __attribute__((aligned(16))) uint8_t hsh[];
    unsigned long long *lkeys = (unsigned long long *)hsh;          /* [L] */
    ThreadAcc *lcells = (ThreadAcc *)(hsh + (size_t)L * sizeof(unsigned long long));

    for (uint32_t i = threadIdx.x; i < L; i += AGG_BLOCK) {
        lkeys[i] = HASH_EMPTY;
        for (uint32_t a = 0; a < n_aggs_ct; a++)
            acc_init(lcells[i * n_aggs_ct + a], params.aggs[a].kind);
    }
    __syncthreads();

    for (uint32_t work = blockIdx.x; work < hp.n_work; work += gridDim.x) {
        const uint32_t gid = work / params.tiles_per_group;
        const uint32_t tile = work % params.tiles_per_group;
        const GroupDesc g = groups[gid];
        const ColLoc *cols = colloc + g.colbase;
        uint32_t row_start = tile * TILE_ROWS;
        uint32_t row_end = min(row_start + TILE_ROWS, g.row_count);

        for (uint32_t base_row = row_start + wid * WAVE; base_row < row_end;
             base_row += WAVE * n_waves) {
            uint32_t row = base_row + lane;
            bool pass = row < row_end;
            if (pass) {
                int last_proj = -1;
                int64_t liv = 0; double lfv = 0; bool lok = false;
                bool gv = false;
                for (uint32_t p = 0; p < params.n_preds; p++) {
                    const PredD &pr = params.preds[p];
                    if ((int)pr.proj != last_proj) {
                        lok = col_value(data, scratch, rank, cols[pr.proj], row, liv, lfv);
                        last_proj = (int)pr.proj;
                    }
                    gv = gv | (lok && pred_eval(pr, liv, lfv));
                    if (pr.gend) { pass = pass & gv; gv = false; }
                }
            }
            if (!pass) continue;
            /* packed key: per column 0 = NULL, else 1 + (v - lo); NULL keys
             * form their own group (HashAggregate treats NULLs as equal) */
            uint64_t key = 0;
            bool in_range = true, bad_text = false;
            for (uint32_t kc = 0; kc < hp.n_key_cols; kc++) {
                int64_t kv; double kf;
                uint64_t code = 0;
                if (col_value(data, scratch, rank, cols[hp.kproj[kc]], row, kv, kf)) {
                    if (hp.klex[kc]) {
                        const uint32_t lex = hash_text_lex((uint32_t)kv);
                        if (hash_text_slot(lex) != (uint32_t)kv) bad_text = true;
                        kv = (int64_t)lex;
                    }
                    const uint64_t d = (uint64_t)kv - (uint64_t)hp.klo[kc];
                    in_range = in_range && d <= hp.kspan[kc];
                    code = d + 1;
                }
                key |= code << hp.kshift[kc];
            }
            if (bad_text) {
                atomicOr(err, HASH_ERR_TEXT);
                continue;
            }
            if (!in_range) {        /* skip nodes lie: fail, never mis-group */
                atomicOr(err, HASH_ERR_RANGE);
                continue;
            }
            const uint64_t h = hash_mix64(key);
            uint32_t lslot = (uint32_t)(h >> 32) & (L - 1);
            bool in_lds = false;
            if (L) {
                for (uint32_t pr = 0; pr < HASH_LDS_PROBES; pr++) {
                    const unsigned long long prev = atomicCAS(&lkeys[lslot], HASH_EMPTY, key);
                    if (prev == HASH_EMPTY || prev == key) { in_lds = true; break; }
                    lslot = (lslot + 1) & (L - 1);
                }
            }
            if (in_lds) {
                ThreadAcc *cell = lcells + (size_t)lslot * n_aggs_ct;
                for (uint32_t a = 0; a < n_aggs_ct; a++) {
                    PrepAcc p;
                    acc_prepare(p, params.aggs[a], data, scratch, rank, cols, row);
                    acc_apply_atomic(&cell[a], params.aggs[a].kind, p);
                }
            } else {
                const uint64_t gs = hash_global_insert(gkeys, hp.slots, h, key, err);
                if (gs == HASH_NONE) continue;
                ThreadAcc *cell = gcells + gs * n_aggs_ct;
                for (uint32_t a = 0; a < n_aggs_ct; a++) {
                    PrepAcc p;
                    acc_prepare(p, params.aggs[a], data, scratch, rank, cols, row);
                    acc_apply_atomic(&cell[a], params.aggs[a].kind, p);
                }
            }
        }
    }
    __syncthreads();

    /* flush: every thread merges the occupied LDS slots it owns into the
     * global table — same insert, then the carry-exact atomic merge */
    for (uint32_t i = threadIdx.x; i < L; i += AGG_BLOCK) {
        const unsigned long long key = lkeys[i];
        if (key == HASH_EMPTY) continue;
        const uint64_t gs = hash_global_insert(gkeys, hp.slots, hash_mix64(key), key, err);
        if (gs == HASH_NONE) continue;
        ThreadAcc *cell = gcells + gs * n_aggs_ct;
        for (uint32_t a = 0; a < n_aggs_ct; a++) {
            const ThreadAcc &t = lcells[i * n_aggs_ct + a];
            const AccCell c{t.lo, t.hi, t.f, t.cnt};
            cell_merge_atomic(&cell[a], params.aggs[a].kind, c);
        }
    }
}

__global__ __launch_bounds__(AGG_BLOCK) void hash_compact_kernel(
    const unsigned long long *__restrict__ gkeys, const ThreadAcc *__restrict__ gcells,
    unsigned long long *__restrict__ count, unsigned long long *__restrict__ okeys,
    AccCell *__restrict__ ocells, uint64_t capacity, const HashParams hp)
{
    const uint32_t n_aggs = hp.base.n_aggs;
    const uint32_t lane = threadIdx.x % WAVE;
    /* wave-uniform trip count: the ballot below needs every lane present */
    for (uint64_t base = (uint64_t)blockIdx.x * AGG_BLOCK; base < hp.slots;
         base += (uint64_t)gridDim.x * AGG_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        unsigned long long key = HASH_EMPTY;
        if (i < hp.slots) key = gkeys[i];
        const bool occ = key != HASH_EMPTY;
        const uint64_t m = __ballot(occ);
        if (m == 0) continue;
        const int leader = __ffsll((unsigned long long)m) - 1;
        unsigned long long wbase = 0;
        if ((int)lane == leader)
            wbase = atomicAdd(count, (unsigned long long)__popcll(m));
        wbase = (unsigned long long)__shfl((long long)wbase, leader, WAVE);
        if (!occ) continue;
        /* the count stays exact past capacity (the host reports it); only
         * the writes are bounded by the destination's size */
        const uint64_t at = wbase + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
        if (at >= capacity) continue;
        okeys[at] = key;
        for (uint32_t a = 0; a < n_aggs; a++) {
            const ThreadAcc t = gcells[i * n_aggs + a];
            const AccCell c{t.lo, t.hi, t.f, t.cnt};
            ocells[at * n_aggs + a] = c;
        }
    }
}

static uint32_t hash_bitlen(uint64_t x)
{
    uint32_t n = 0;
    while (x) { n++; x >>= 1; }
    return n;
}

/* grow-only device buffer: reallocates when `need` elements exceed `have` */
template <typename T>
static int hash_grow(T *&ptr, uint64_t &have, uint64_t need)
{
    if (need <= have && ptr) return CSTRIPE_OK;
    if (ptr) HIP_TRY(hipFree(ptr));
    ptr = nullptr;
    have = 0;
    HIP_TRY(hipMalloc(&ptr, need * sizeof(T)));
    have = need;
    return CSTRIPE_OK;
}

/* what the front half shared by csgpu_agg_hashed and csgpu_agg_hashed_topn
 * leaves behind: the key packing, and `n` compacted groups in d_hokeys /
 * d_hocells */
struct HashFront {
    HashParams hp;
    uint32_t kbits[CSTRIPE_MAX_HASH_KEY_COLS];
    uint64_t n;
};

/* front half, host part: argument checks and key packing; no device work */
static int hash_prepare(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                        const uint32_t *key_cols, uint32_t n_key_cols,
                        uint64_t capacity, const cstripe_hgroups *out, HashFront &hf)
{
    cstripe_reader *r = s->r;
    hf = HashFront{};
    HashParams &hp = hf.hp;
    uint32_t *kbits = hf.kbits;
    if (!aggs || !out || !key_cols || n_aggs == 0) { cs_set_err("scan_agg_hashed: bad args"); return CSTRIPE_ERR_ARG; }
    if (n_aggs > MAX_AGGS) { cs_set_err("too many aggs"); return CSTRIPE_ERR_ARG; }
    if (s->preds.size() > MAX_PREDS) { cs_set_err("too many preds"); return CSTRIPE_ERR_ARG; }
    if (n_key_cols == 0 || n_key_cols > CSTRIPE_MAX_HASH_KEY_COLS) {
        cs_set_err("scan_agg_hashed: %u key columns (1..%d; zero keys is cstripe_scan_agg)",
                   n_key_cols, CSTRIPE_MAX_HASH_KEY_COLS);
        return CSTRIPE_ERR_ARG;
    }
    if (capacity == 0 || capacity > CSTRIPE_MAX_HASH_GROUPS) {
        cs_set_err("scan_agg_hashed: capacity %llu outside 1..%u",
                   (unsigned long long)capacity, CSTRIPE_MAX_HASH_GROUPS);
        return CSTRIPE_ERR_ARG;
    }
    if (!out->partials) { cs_set_err("scan_agg_hashed: no partials destination"); return CSTRIPE_ERR_ARG; }

    AggParams &p = hp.base;
    for (uint32_t i = 0; i < n_aggs; i++)
        if (aggs[i].kind > CSTRIPE_AGG_SUM_DISC_TAX_I64) { cs_set_err("agg %u: bad kind %u", i, aggs[i].kind); return CSTRIPE_ERR_ARG; }
    { int _rc = fill_agg_params(s, aggs, n_aggs, p); if (_rc != CSTRIPE_OK) return _rc; }

    /* key packing: [lo, hi] per key column from the SELECTED chunk groups'
     * skip nodes; total bits <= 63 keeps ~0ull free as the EMPTY marker */
    hp.n_key_cols = n_key_cols;
    bool ktext[CSTRIPE_MAX_HASH_KEY_COLS] = {false};
    uint32_t total_bits = 0;
    auto set_range = [&](uint32_t k, uint32_t col, bool full, int64_t tlo, int64_t thi) {
        int64_t lo = 0, hi = 0;
        bool any = false;
        uint32_t pl = 0;
        if (const cs_lookup *lk = cs_col_lookup(s, col, &pl)) {
            /* a derived column: the [min, max] of its payload array */
            full = true;
            tlo = lk->n ? lk->plo[pl] : 0;
            thi = lk->n ? lk->phi[pl] : 0;
        } else if (const cs_expr *ex = cs_col_expr(s, col)) {
            /* a computed column: the [min, max] its evaluation measured */
            full = true;
            tlo = ex->lo;
            thi = ex->hi;
        } else
        for (const cs_selchunk &sc : s->sel) {
            const csf_skipnode &nd = r->stripes[sc.stripe].nodes[col][sc.chunk].n;
            if (nd.has_min_max) {
                if (!any) { lo = nd.min_i; hi = nd.max_i; any = true; }
                else { lo = std::min(lo, nd.min_i); hi = std::max(hi, nd.max_i); }
            } else if (nd.n_present > 0) {
                full = true;
            }
        }
        if (full) { lo = tlo; hi = thi; }
        if (hi < lo) { lo = 0; hi = 0; }
        hp.klo[k] = lo;
        hp.kspan[k] = (uint64_t)hi - (uint64_t)lo;
        kbits[k] = hp.kspan[k] == ~0ull ? 65u : hash_bitlen(hp.kspan[k] + 1);
    };
    for (uint32_t k = 0; k < n_key_cols; k++) {
        const uint32_t col = key_cols[k];
        const int pj = proj_of(s, (int32_t)col);
        if (like_stream_refused(s, col, "scan_agg_hashed key")) return CSTRIPE_ERR_ARG;
        if (pj < 0) { cs_set_err("scan_agg_hashed: key col %u not projected", col); return CSTRIPE_ERR_ARG; }
        if (!out->keys[k] || !out->key_nulls[k]) { cs_set_err("scan_agg_hashed: no destination for key col %u", k); return CSTRIPE_ERR_ARG; }
        const uint8_t t = cs_col_type(s, col);
        int64_t tlo, thi;
        switch (t) {
            case CSTRIPE_I8:   tlo = INT8_MIN;  thi = INT8_MAX;  break;
            case CSTRIPE_I16:  tlo = INT16_MIN; thi = INT16_MAX; break;
            case CSTRIPE_I32:  tlo = INT32_MIN; thi = INT32_MAX; break;
            case CSTRIPE_I64:  tlo = INT64_MIN; thi = INT64_MAX; break;
            case CSTRIPE_TEXT: tlo = 0;         thi = (int64_t)UINT32_MAX; break;
            case CSTRIPE_VARTEXT: {
                /* the key is the dictionary rank: exactly [0, n_dict - 1]
                 * (the skip nodes hold prefix keys, not ranks) */
                const int64_t nd = (int64_t)s->text_dicts[col].offsets.size() - 1;
                tlo = 0;
                thi = nd > 0 ? nd - 1 : 0;
                break;
            }
            default:
                cs_set_err("scan_agg_hashed: key col %u must be I8/I16/I32/I64/TEXT", col);
                return CSTRIPE_ERR_ARG;
        }
        hp.kproj[k] = (uint32_t)pj;
        ktext[k] = t == CSTRIPE_TEXT;
        set_range(k, col, ktext[k] || t == CSTRIPE_VARTEXT, tlo, thi);
        total_bits += kbits[k];
    }
    if (total_bits > 63) {
        /* beyond the 33-bit whole-slot packing: a TEXT key column may pack
         * by its C-collation order key instead, whose [min, max] the skip
         * nodes do record (canonical short-varlena slots only; the kernel
         * checks every slot and the call fails otherwise) */
        total_bits = 0;
        for (uint32_t k = 0; k < n_key_cols; k++) {
            if (ktext[k]) {
                hp.klex[k] = 1;
                set_range(k, key_cols[k], false, 0, 0xFFFFFF);
            }
            total_bits += kbits[k];
        }
    }
    for (uint32_t k = 0, sh = 0; k < n_key_cols && total_bits <= 63; k++) {
        hp.kshift[k] = sh;
        sh += kbits[k];
    }
    if (total_bits > 63) {
        char msg[160];
        int w = 0;
        for (uint32_t k = 0; k < n_key_cols; k++)
            w += snprintf(msg + w, sizeof(msg) - (size_t)w, "%scol %u: %u bits",
                          k ? ", " : "", key_cols[k], kbits[k]);
        cs_set_err("scan_agg_hashed: packed key needs %u bits > 63 (%s) — key ranges "
                   "come from the selected chunk groups' min/max", total_bits, msg);
        return CSTRIPE_ERR_ARG;
    }
    return CSTRIPE_OK;
}

/* front half, device part: decode, hash_init_kernel, hash_agg_kernel and
 * hash_compact_kernel on the scan's stream, the count's copy-back, the
 * device flags and the capacity check; hf.n = compacted groups (0 for an
 * empty selection) */
static int hash_execute(cstripe_scan *s, uint32_t n_aggs, uint64_t capacity, HashFront &hf)
{
    cs_gpu_state *g = s->gpu;
    HashParams &hp = hf.hp;
    const AggParams &p = hp.base;
    hf.n = 0;
    hp.n_work = g->n_groups * p.tiles_per_group;
    if (hp.n_work == 0) {
        s->last_kernel_ms = s->last_decode_ms = s->last_agg_ms = 0;
        s->last_hash_init_ms = s->last_hash_scan_ms = s->last_hash_compact_ms = 0;
        return CSTRIPE_OK;
    }

    uint64_t slots = 2;
    while (slots < 2 * capacity) slots <<= 1;
    hp.slots = slots;

    /* LDS table: the largest power of two whose key words + cells fit the
     * byte budget; CSTRIPE_HASH_LDS_SLOTS (read per call) overrides it */
    const uint32_t slot_bytes = (uint32_t)sizeof(unsigned long long) +
                                n_aggs * (uint32_t)sizeof(ThreadAcc);
    uint32_t lds_max = 1;
    while (lds_max * 2 * slot_bytes <= HASH_LDS_BUDGET) lds_max *= 2;
    uint32_t lds_slots = lds_max;
    if (const char *e = getenv("CSTRIPE_HASH_LDS_SLOTS")) {
        const long v = atol(e);
        if (v <= 0) lds_slots = 0;
        else {
            lds_slots = 1;
            while ((long)lds_slots * 2 <= v && lds_slots * 2 <= lds_max) lds_slots *= 2;
        }
    }
    hp.lds_slots = lds_slots;
    const uint32_t lds_bytes = lds_slots * slot_bytes;

    for (hipEvent_t &e : g->hev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    { int _rc = hash_grow(g->d_hkeys, g->hkeys_slots, slots); if (_rc != CSTRIPE_OK) return _rc; }
    { int _rc = hash_grow(g->d_hcells, g->hcells_n, slots * n_aggs); if (_rc != CSTRIPE_OK) return _rc; }
    { int _rc = hash_grow(g->d_hokeys, g->hokeys_n, capacity); if (_rc != CSTRIPE_OK) return _rc; }
    { int _rc = hash_grow(g->d_hocells, g->hocells_n, capacity * n_aggs); if (_rc != CSTRIPE_OK) return _rc; }
    if (!g->d_hcount) HIP_TRY(hipMalloc(&g->d_hcount, sizeof(unsigned long long)));

    const uint32_t grid = hp.n_work < HASH_GRID ? hp.n_work : HASH_GRID;
    const uint64_t table_blocks = (slots + AGG_BLOCK - 1) / AGG_BLOCK;
    const uint32_t tgrid = (uint32_t)(table_blocks < 4096 ? table_blocks : 4096);

    HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
    HIP_TRY(hipEventRecord(g->hev[0], g->stream));
    { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
    HIP_TRY(hipEventRecord(g->hev[1], g->stream));
    hipLaunchKernelGGL(hash_init_kernel, dim3(tgrid), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_hkeys, g->d_hcells, g->d_hcount, hp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->hev[2], g->stream));
    {
        auto launchh = [&](auto *kern) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(AGG_BLOCK), lds_bytes, g->stream,
                               g->d_data, g->d_scratch, g->d_rank, g->d_groups,
                               g->d_colloc, g->d_hkeys, g->d_hcells, g->d_error, hp);
        };
        if (n_aggs == 5) launchh(hash_agg_kernel<5>);
        else if (n_aggs == 1) launchh(hash_agg_kernel<1>);
        else if (n_aggs == 2) launchh(hash_agg_kernel<2>);
        else launchh(hash_agg_kernel<-1>);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(g->hev[3], g->stream));
    hipLaunchKernelGGL(hash_compact_kernel, dim3(tgrid), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_hkeys, g->d_hcells, g->d_hcount, g->d_hokeys, g->d_hocells,
                       capacity, hp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->hev[4], g->stream));

    /* the count's copy-back is the only sync before the result copy */
    unsigned long long h_n = 0;
    int h_err = 0;
    HIP_TRY(hipMemcpyAsync(&h_n, g->d_hcount, sizeof(h_n), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    float ms_d = 0, ms_i = 0, ms_s = 0, ms_c = 0;
    (void)hipEventElapsedTime(&ms_d, g->hev[0], g->hev[1]);
    (void)hipEventElapsedTime(&ms_i, g->hev[1], g->hev[2]);
    (void)hipEventElapsedTime(&ms_s, g->hev[2], g->hev[3]);
    (void)hipEventElapsedTime(&ms_c, g->hev[3], g->hev[4]);
    s->last_decode_ms = ms_d;
    s->last_hash_init_ms = ms_i;
    s->last_hash_scan_ms = ms_s;
    s->last_hash_compact_ms = ms_c;
    s->last_agg_ms = ms_i + ms_s + ms_c;
    s->last_kernel_ms = ms_d + ms_i + ms_s + ms_c;
    s->last_fused = 0;
    if (h_err & 4) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    if (h_err & HASH_ERR_RANGE) {
        cs_set_err("scan_agg_hashed: a key value lies outside its chunk's recorded min/max "
                   "(device flag %d) — corrupt skip nodes", h_err);
        return CSTRIPE_ERR_FORMAT;
    }
    if (h_err & HASH_ERR_TEXT) {
        cs_set_err("scan_agg_hashed: a TEXT key slot is not a canonical short varlena, so the "
                   "key tuple cannot pack by order key (whole-slot packing needs more than 63 bits)");
        return CSTRIPE_ERR_ARG;
    }
    if (h_err & HASH_ERR_FULL) {
        cs_set_err("scan_agg_hashed: more than %llu groups (hash table full; capacity %llu)",
                   (unsigned long long)slots, (unsigned long long)capacity);
        return CSTRIPE_ERR_ARG;
    }
    if (h_err) { cs_set_err("scan_agg_hashed: device flag %d", h_err); return CSTRIPE_ERR; }
    if (h_n > capacity) {
        cs_set_err("scan_agg_hashed: %llu groups > capacity %llu",
                   h_n, (unsigned long long)capacity);
        return CSTRIPE_ERR_ARG;
    }
    hf.n = h_n;
    return CSTRIPE_OK;
}

int csgpu_agg_hashed(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                     const uint32_t *key_cols, uint32_t n_key_cols,
                     uint64_t capacity, cstripe_hgroups *out)
{
    if (!s->gpu) { cs_set_err("scan not staged — call cstripe_gpu_stage first (GPU required; no CPU fallback)"); return CSTRIPE_ERR_NOGPU; }
    cs_gpu_state *g = s->gpu;
    HashFront hf;
    { int _rc = hash_prepare(s, aggs, n_aggs, key_cols, n_key_cols, capacity, out, hf); if (_rc != CSTRIPE_OK) return _rc; }
    { int _rc = hash_execute(s, n_aggs, capacity, hf); if (_rc != CSTRIPE_OK) return _rc; }
    const HashParams &hp = hf.hp;
    const uint32_t *kbits = hf.kbits;
    const uint64_t n = hf.n;
    if (n == 0) { out->n_groups = 0; return CSTRIPE_OK; }

    std::vector<unsigned long long> h_keys(n);
    std::vector<AccCell> h_cells((size_t)n * n_aggs);
    HIP_TRY(hipMemcpyAsync(h_keys.data(), g->d_hokeys, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(h_cells.data(), g->d_hocells, h_cells.size() * sizeof(AccCell), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));

    /* unpack, then sort ascending by key tuple: column 0 most significant,
     * signed compare, per column NULL last (PG ASC = NULLS LAST) */
    auto code_of = [&](unsigned long long key, uint32_t k) -> uint64_t {
        const uint64_t m = kbits[k] >= 64 ? ~0ull : ((1ull << kbits[k]) - 1ull);
        return (key >> hp.kshift[k]) & m;
    };
    auto value_of = [&](uint64_t code, uint32_t k) -> int64_t {
        const int64_t v = (int64_t)((uint64_t)hp.klo[k] + (code - 1));
        return hp.klex[k] ? (int64_t)hash_text_slot((uint32_t)v) : v;
    };
    std::vector<int64_t> kval[CSTRIPE_MAX_HASH_KEY_COLS];
    std::vector<uint8_t> knull[CSTRIPE_MAX_HASH_KEY_COLS];
    for (uint32_t k = 0; k < n_key_cols; k++) {
        kval[k].resize(n);
        knull[k].resize(n);
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t code = code_of(h_keys[i], k);
            knull[k][i] = code == 0 ? 1 : 0;
            kval[k][i] = code == 0 ? 0 : value_of(code, k);
        }
    }
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        for (uint32_t k = 0; k < n_key_cols; k++) {
            if (knull[k][a] != knull[k][b]) return knull[k][a] < knull[k][b];   /* NULL last */
            if (kval[k][a] != kval[k][b]) return kval[k][a] < kval[k][b];
        }
        return false;
    });
    for (uint64_t oi = 0; oi < n; oi++) {
        const uint64_t i = order[oi];
        for (uint32_t k = 0; k < n_key_cols; k++) {
            out->key_nulls[k][oi] = knull[k][i];
            out->keys[k][oi] = kval[k][i];
        }
        for (uint32_t a = 0; a < n_aggs; a++)
            out->partials[(size_t)oi * n_aggs + a] =
                cell_to_partial(aggs[a].kind, h_cells[(size_t)i * n_aggs + a]);
    }
    out->n_groups = n;
    return CSTRIPE_OK;
}

/* =====================================================================
 * scan_select_topn — device ORDER BY ... LIMIT over the scan: what the
 * reference pushes to every worker (WorkerSortClauseList / WorkerLimitCount,
 * multi_logical_optimizer.c:5038-5212: each shard runs ORDER BY ... LIMIT
 * limit+offset, the coordinator re-sorts the few rows it gets back).
 *
 * The pass mask, tile counts and bases of scan_select are reused READ-ONLY;
 * everything refined lives in the d_tn_* buffers. On the scan's stream:
 *
 *   topn_key_kernel      one block per chunk group x TILE_ROWS tile (the
 *                        select grid). Each passing row's order tuple packs
 *                        into ONE 64-bit word whose unsigned order is the
 *                        requested order, stored at bases[tile] + rank in
 *                        tile — scan order, select_emit_kernel's arithmetic.
 *   radix select         MSB first, 8 bits per round, ceil(bits/8) rounds:
 *     topn_hist_kernel   capped grid, grid-stride over the key array; a
 *                        256-bin LDS histogram of the round's digit over the
 *                        keys whose higher digits equal the prefix so far,
 *                        nonzero bins flushed with one global atomicAdd each
 *     topn_pick_kernel   one wave: scans the 256 bins, finds the bin where
 *                        the running count crosses the remaining k, extends
 *                        the prefix, lowers k, clears the bins
 *                        After the last round prefix = T, the exact key of
 *                        the limit-th smallest row, and k = ties on T needed.
 *   topn_refine_kernel   per tile: key < T words, key == T words, tie count
 *   select_offsets_kernel  over the tie counts
 *   topn_final_kernel    per tile: lt | (eq & tie ordinal < ties needed),
 *                        final counts; ties are taken by scan-order prefix,
 *                        which is the ascending-row-number tie-break
 *   select_offsets_kernel  over the final counts
 *   select_emit_kernel   unchanged, over the refined mask and bases: exactly
 *                        `limit` rows in scan order
 *   topn_keygather_kernel  their keys alongside
 *   (host)               one DtoH copy of `limit` keys, a stable sort
 *   topn_permute_kernel  values / null bytes / row numbers into final order
 *
 * No flag, fence, spin-wait or cross-block dependency exists inside a
 * kernel; the stages are ordered by kernel boundaries on the stream. The
 * only global words several blocks touch are the 256 histogram bins, updated
 * by integer atomicAdd alone, so nothing depends on arrival order. Every
 * loop is bounded by the key count, the tile size or a constant.
 * ===================================================================== */

#define TOPN_GRID       2048
#define TOPN_ERR_RANGE  1024            /* key outside its skip-node range */
#define TOPN_SIGN       0x8000000000000000ull
#define TOPN_F_DESC     1u
#define TOPN_F_NFIRST   2u
#define TOPN_F_FLOAT    4u

struct TopnParams {
    uint32_t n_order, tiles_per_group;
    uint32_t kproj[CSTRIPE_MAX_ORDER_COLS];
    uint32_t kshift[CSTRIPE_MAX_ORDER_COLS];
    uint32_t kflags[CSTRIPE_MAX_ORDER_COLS];
    uint64_t klo[CSTRIPE_MAX_ORDER_COLS];     /* ord(lo) */
    uint64_t kspan[CSTRIPE_MAX_ORDER_COLS];   /* ord(hi) - ord(lo) */
    uint64_t n_keys;
};

struct TopnState {
    unsigned long long prefix;          /* digits found so far; T at the end */
    unsigned long long k;               /* rank still wanted inside the prefix */
    unsigned long long hist[256];
};

/* order-preserving map of an f64 to u64 under PG float order: every NaN is
 * one code above +inf, -0.0 is +0.0 (float8_cmp_internal) */
__host__ __device__ inline uint64_t topn_f64_ord(double v)
{
    if (v != v) return 0xFFF0000000000001ull;
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    if (u == TOPN_SIGN) u = 0;
    return (u >> 63) ? ~u : (u | TOPN_SIGN);
}

/* mask words of one tile into LDS plus the passing rows in earlier slices
 * (wave `wid` does it; SEL_SLICES == WAVE, one lane per word) */
__device__ inline void topn_load_words(const uint64_t *__restrict__ mask,
                                       uint64_t *s_word, uint32_t *s_pre, uint32_t lane)
{
    const uint64_t w = mask[(uint64_t)blockIdx.x * SEL_SLICES + lane];
    const uint32_t pc = (uint32_t)__popcll(w);
    uint32_t inc = pc;
    #pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, WAVE);
        if ((int)lane >= d) inc += t;
    }
    s_word[lane] = w;
    s_pre[lane] = inc - pc;
}

__global__ __launch_bounds__(AGG_BLOCK) void topn_key_kernel(
    const uint8_t *__restrict__ data, const uint8_t *__restrict__ scratch,
    const uint32_t *__restrict__ rank, const GroupDesc *__restrict__ groups,
    const ColLoc *__restrict__ colloc, const uint64_t *__restrict__ mask,
    const uint64_t *__restrict__ bases, uint64_t *__restrict__ keys,
    int *err, const TopnParams tp)
{
    __shared__ uint64_t s_word[SEL_SLICES];
    __shared__ uint32_t s_pre[SEL_SLICES];
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (wid == 0) topn_load_words(mask, s_word, s_pre, lane);
    __syncthreads();

    const uint32_t gid = blockIdx.x / tp.tiles_per_group;
    const uint32_t tile = blockIdx.x % tp.tiles_per_group;
    const ColLoc *cols = colloc + groups[gid].colbase;
    const uint64_t tile_base = bases[blockIdx.x];

    for (uint32_t sl = wid; sl < SEL_SLICES; sl += AGG_BLOCK / WAVE) {
        const uint64_t word = s_word[sl];
        const uint64_t bit = 1ull << lane;
        if (!(word & bit)) continue;
        const uint32_t row = tile * TILE_ROWS + sl * WAVE + lane;
        const uint64_t idx = tile_base + s_pre[sl] +
                             (uint32_t)__popcll(word & (bit - 1));
        /* per column: d = ord(v) - ord(lo) in [0, span], reversed for DESC;
         * NULL takes the code below (NULLS FIRST) or above all values */
        uint64_t key = 0;
        bool in_range = true;
        for (uint32_t kc = 0; kc < tp.n_order; kc++) {
            const uint32_t fl = tp.kflags[kc];
            int64_t kv; double kf;
            uint64_t code;
            if (col_value(data, scratch, rank, cols[tp.kproj[kc]], row, kv, kf)) {
                const uint64_t o = (fl & TOPN_F_FLOAT) ? topn_f64_ord(kf)
                                                       : ((uint64_t)kv ^ TOPN_SIGN);
                uint64_t d = o - tp.klo[kc];
                if (d > tp.kspan[kc]) { in_range = false; d = 0; }
                if (fl & TOPN_F_DESC) d = tp.kspan[kc] - d;
                code = (fl & TOPN_F_NFIRST) ? d + 1 : d;
            } else {
                code = (fl & TOPN_F_NFIRST) ? 0 : tp.kspan[kc] + 1;
            }
            key |= code << tp.kshift[kc];
        }
        if (!in_range) atomicOr(err, TOPN_ERR_RANGE);   /* skip nodes lie */
        if (idx < tp.n_keys) keys[idx] = key;
    }
}

__global__ __launch_bounds__(AGG_BLOCK) void topn_init_kernel(TopnState *st, uint64_t k)
{
    st->hist[threadIdx.x] = 0;          /* AGG_BLOCK == 256 bins */
    if (threadIdx.x == 0) { st->prefix = 0; st->k = k; }
}

__global__ __launch_bounds__(AGG_BLOCK) void topn_hist_kernel(
    const uint64_t *__restrict__ keys, uint64_t n, TopnState *st, uint32_t shift)
{
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t prefix = st->prefix;
    const bool top = shift + 8 >= 64;           /* no higher digits */
    const uint32_t hs = top ? 0 : shift + 8;
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * AGG_BLOCK) {
        const uint64_t key = keys[i];
        if (top || (key >> hs) == prefix)
            atomicAdd(&lh[(key >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    if (c) atomicAdd(&st->hist[threadIdx.x], (unsigned long long)c);
}

__global__ __launch_bounds__(WAVE) void topn_pick_kernel(TopnState *st)
{
    const uint32_t lane = threadIdx.x;
    unsigned long long c[4], sum = 0;
    #pragma unroll
    for (uint32_t j = 0; j < 4; j++) { c[j] = st->hist[lane * 4 + j]; sum += c[j]; }
    const unsigned long long k = st->k;
    const unsigned long long prefix = st->prefix;
    unsigned long long inc = sum;
    #pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned long long t = (unsigned long long)__shfl_up((long long)inc, d, WAVE);
        if ((int)lane >= d) inc += t;
    }
    unsigned long long run = inc - sum;
    #pragma unroll
    for (uint32_t j = 0; j < 4; j++) st->hist[lane * 4 + j] = 0;
    if (run < k && k <= inc) {          /* exactly one lane: the crossing */
        #pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (k <= run + c[j]) {
                st->prefix = (prefix << 8) | (lane * 4 + j);
                st->k = k - run;
                break;
            }
            run += c[j];
        }
    }
}

__global__ __launch_bounds__(AGG_BLOCK) void topn_refine_kernel(
    const uint64_t *__restrict__ mask, const uint64_t *__restrict__ bases,
    const uint64_t *__restrict__ keys, uint64_t n_keys,
    const TopnState *__restrict__ st, uint64_t *__restrict__ lt_mask,
    uint64_t *__restrict__ eq_mask, uint32_t *__restrict__ tie_counts)
{
    __shared__ uint64_t s_word[SEL_SLICES];
    __shared__ uint32_t s_pre[SEL_SLICES];
    __shared__ uint32_t s_cnt[AGG_BLOCK / WAVE];
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (wid == 0) topn_load_words(mask, s_word, s_pre, lane);
    __syncthreads();
    const uint64_t T = st->prefix;
    const uint64_t tile_base = bases[blockIdx.x];
    uint32_t wcount = 0;
    for (uint32_t sl = wid; sl < SEL_SLICES; sl += AGG_BLOCK / WAVE) {
        const uint64_t word = s_word[sl];
        const uint64_t bit = 1ull << lane;
        bool lt = false, eq = false;
        if (word & bit) {
            const uint64_t idx = tile_base + s_pre[sl] +
                                 (uint32_t)__popcll(word & (bit - 1));
            if (idx < n_keys) {
                const uint64_t key = keys[idx];
                lt = key < T;
                eq = key == T;
            }
        }
        const uint64_t ltw = __ballot(lt), eqw = __ballot(eq);
        if (lane == 0) {
            lt_mask[(uint64_t)blockIdx.x * SEL_SLICES + sl] = ltw;
            eq_mask[(uint64_t)blockIdx.x * SEL_SLICES + sl] = eqw;
        }
        wcount += (uint32_t)__popcll(eqw);
    }
    if (lane == 0) s_cnt[wid] = wcount;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < AGG_BLOCK / WAVE; w++) c += s_cnt[w];
        tie_counts[blockIdx.x] = c;
    }
}

/* fin_mask holds the key < T words on entry and the final words on exit:
 * each word is read and rewritten by the one wave that owns its slice */
__global__ __launch_bounds__(AGG_BLOCK) void topn_final_kernel(
    const uint64_t *__restrict__ eq_mask, const uint64_t *__restrict__ tie_bases,
    const TopnState *__restrict__ st, uint64_t *fin_mask,
    uint32_t *__restrict__ counts)
{
    __shared__ uint64_t s_word[SEL_SLICES];
    __shared__ uint32_t s_pre[SEL_SLICES];
    __shared__ uint32_t s_cnt[AGG_BLOCK / WAVE];
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (wid == 0) topn_load_words(eq_mask, s_word, s_pre, lane);
    __syncthreads();
    const uint64_t need = st->k;
    const uint64_t tie_base = tie_bases[blockIdx.x];
    uint32_t wcount = 0;
    for (uint32_t sl = wid; sl < SEL_SLICES; sl += AGG_BLOCK / WAVE) {
        const uint64_t eqw = s_word[sl];
        const uint64_t bit = 1ull << lane;
        const uint64_t ordinal = tie_base + s_pre[sl] +
                                 (uint32_t)__popcll(eqw & (bit - 1));
        const bool take = (eqw & bit) && ordinal < need;
        const uint64_t ltw = fin_mask[(uint64_t)blockIdx.x * SEL_SLICES + sl];
        const uint64_t fin = ltw | __ballot(take);
        if (lane == 0) fin_mask[(uint64_t)blockIdx.x * SEL_SLICES + sl] = fin;
        wcount += (uint32_t)__popcll(fin);
    }
    if (lane == 0) s_cnt[wid] = wcount;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < AGG_BLOCK / WAVE; w++) c += s_cnt[w];
        counts[blockIdx.x] = c;
    }
}

/* keys of the rows the final mask keeps, at their emit position */
__global__ __launch_bounds__(AGG_BLOCK) void topn_keygather_kernel(
    const uint64_t *__restrict__ mask, const uint64_t *__restrict__ bases,
    const uint64_t *__restrict__ fin_mask, const uint64_t *__restrict__ fin_bases,
    const uint64_t *__restrict__ keys, uint64_t n_keys,
    uint64_t *__restrict__ okeys, uint64_t n_out)
{
    __shared__ uint64_t s_word[SEL_SLICES], s_fword[SEL_SLICES];
    __shared__ uint32_t s_pre[SEL_SLICES], s_fpre[SEL_SLICES];
    const uint32_t wid = threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x % WAVE;
    if (wid == 0) topn_load_words(mask, s_word, s_pre, lane);
    if (wid == 1) topn_load_words(fin_mask, s_fword, s_fpre, lane);
    __syncthreads();
    const uint64_t tile_base = bases[blockIdx.x];
    const uint64_t fin_base = fin_bases[blockIdx.x];
    for (uint32_t sl = wid; sl < SEL_SLICES; sl += AGG_BLOCK / WAVE) {
        const uint64_t fw = s_fword[sl];
        const uint64_t bit = 1ull << lane;
        if (!(fw & bit)) continue;
        const uint64_t src = tile_base + s_pre[sl] +
                             (uint32_t)__popcll(s_word[sl] & (bit - 1));
        const uint64_t dst = fin_base + s_fpre[sl] +
                             (uint32_t)__popcll(fw & (bit - 1));
        if (src < n_keys && dst < n_out) okeys[dst] = keys[src];
    }
}

struct PermCol {
    const uint8_t *src_vals;
    uint8_t *dst_vals;
    const uint8_t *src_nulls;   /* or nullptr */
    uint8_t *dst_nulls;
    uint32_t width;
    uint32_t pad;
};

struct PermParams {
    uint32_t n_cols, pad;
    uint64_t n;
    const uint64_t *src_rn;     /* or nullptr */
    uint64_t *dst_rn;
    PermCol cols[MAX_PROJ];
};

__global__ __launch_bounds__(AGG_BLOCK) void topn_permute_kernel(
    const uint32_t *__restrict__ perm, const PermParams pp)
{
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; i < pp.n;
         i += (uint64_t)gridDim.x * AGG_BLOCK) {
        const uint64_t src = perm[i];
        if (src >= pp.n) continue;
        if (pp.src_rn) pp.dst_rn[i] = pp.src_rn[src];
        for (uint32_t c = 0; c < pp.n_cols; c++) {
            const PermCol &pc = pp.cols[c];
            switch (pc.width) {
                case 1: pc.dst_vals[i] = pc.src_vals[src]; break;
                case 2: ((uint16_t *)pc.dst_vals)[i] = ((const uint16_t *)pc.src_vals)[src]; break;
                case 4: ((uint32_t *)pc.dst_vals)[i] = ((const uint32_t *)pc.src_vals)[src]; break;
                default: ((uint64_t *)pc.dst_vals)[i] = ((const uint64_t *)pc.src_vals)[src]; break;
            }
            if (pc.src_nulls) pc.dst_nulls[i] = pc.src_nulls[src];
        }
    }
}

static void topn_zero_timing(cstripe_scan *s)
{
    select_zero_timing(s);
    s->last_topn_key_ms = s->last_topn_select_ms = s->last_topn_emit_ms = 0;
}

int csgpu_select_topn(cstripe_scan *s, const cstripe_order_key *order, uint32_t n_order,
                      uint64_t limit, cstripe_rows *out, int dst_on_device)
{
    if (!s->gpu) { cs_set_err("scan not staged — call cstripe_gpu_stage first (GPU required; no CPU fallback)"); return CSTRIPE_ERR_NOGPU; }
    cs_gpu_state *g = s->gpu;
    cstripe_reader *r = s->r;
    const uint32_t n_cols = cs_scan_ncols(s);
    if (!order || !out) { cs_set_err("scan_select_topn: bad args"); return CSTRIPE_ERR_ARG; }
    if (limit == 0 || limit > CSTRIPE_MAX_TOPN) {
        cs_set_err("scan_select_topn: limit %llu outside 1..%u",
                   (unsigned long long)limit, CSTRIPE_MAX_TOPN);
        return CSTRIPE_ERR_ARG;
    }
    if (n_order == 0 || n_order > CSTRIPE_MAX_ORDER_COLS) {
        cs_set_err("scan_select_topn: %u order columns (1..%d)", n_order, CSTRIPE_MAX_ORDER_COLS);
        return CSTRIPE_ERR_ARG;
    }

    TopnParams tp{};
    tp.n_order = n_order;
    uint8_t otype[CSTRIPE_MAX_ORDER_COLS] = {0};
    for (uint32_t k = 0; k < n_order; k++) {
        const uint32_t col = order[k].column;
        if (like_stream_refused(s, col, "scan_select_topn order")) return CSTRIPE_ERR_ARG;
        if (proj_of(s, (int32_t)col) < 0) {
            cs_set_err("scan_select_topn: order col %u not projected", col);
            return CSTRIPE_ERR_ARG;
        }
        for (uint32_t j = 0; j < k; j++)
            if (order[j].column == col) {
                cs_set_err("scan_select_topn: order col %u repeated", col);
                return CSTRIPE_ERR_ARG;
            }
        if (order[k].flags & ~(CSTRIPE_ORDER_DESC | CSTRIPE_ORDER_NULLS_FIRST)) {
            cs_set_err("scan_select_topn: order col %u: unknown flags 0x%x", col, order[k].flags);
            return CSTRIPE_ERR_ARG;
        }
        const uint8_t t = cs_col_type(s, col);
        if (t == CSTRIPE_TEXT) {
            cs_set_err("scan_select_topn: order col %u is TEXT — its row-level order in this "
                       "ABI is whole-slot, not collation; order by a VARTEXT column instead", col);
            return CSTRIPE_ERR_ARG;
        }
        if (t < CSTRIPE_I8 || t > CSTRIPE_VARTEXT) {
            cs_set_err("scan_select_topn: order col %u must be I8/I16/I32/I64/F32/F64/VARTEXT", col);
            return CSTRIPE_ERR_ARG;
        }
        otype[k] = t;
        tp.kproj[k] = (uint32_t)g->proj_of_col[col];
        tp.kflags[k] = ((order[k].flags & CSTRIPE_ORDER_DESC) ? TOPN_F_DESC : 0u) |
                       ((order[k].flags & CSTRIPE_ORDER_NULLS_FIRST) ? TOPN_F_NFIRST : 0u) |
                       ((t == CSTRIPE_F32 || t == CSTRIPE_F64) ? TOPN_F_FLOAT : 0u);
    }

    SelectParams sp{};
    uint8_t widths[MAX_PROJ] = {0};
    uint32_t dst_col[MAX_PROJ] = {0};
    for (uint32_t c = 0; c < n_cols && out->col_values; c++) {
        if (!out->col_values[c]) continue;
        const int pj = proj_of(s, (int32_t)c);
        if (like_stream_refused(s, c, "scan_select_topn")) return CSTRIPE_ERR_ARG;
        if (pj < 0) { cs_set_err("scan_select_topn: column %u not projected", c); return CSTRIPE_ERR_ARG; }
        widths[sp.n_cols] = (uint8_t)csf_type_width(cs_col_type(s, c));
        dst_col[sp.n_cols] = c;
        sp.cols[sp.n_cols].proj = (uint32_t)pj;
        sp.n_cols++;
    }

    /* key packing: per column [ord(lo), ord(hi)] from the SELECTED chunk
     * groups' skip nodes (ints biased to unsigned, floats through
     * topn_f64_ord — their min/max are recorded in PG order already);
     * bitlen(span + 1) bits hold the value offsets and one NULL code */
    uint32_t kbits[CSTRIPE_MAX_ORDER_COLS] = {0};
    uint32_t total_bits = 0;
    for (uint32_t k = 0; k < n_order; k++) {
        const uint32_t col = order[k].column;
        const uint8_t t = otype[k];
        const bool is_f = (tp.kflags[k] & TOPN_F_FLOAT) != 0;
        auto ord_i = [](int64_t v) -> uint64_t { return (uint64_t)v ^ TOPN_SIGN; };
        auto ord_node = [&](int64_t bits_or_val) -> uint64_t {
            if (!is_f) return ord_i(bits_or_val);
            double d;
            memcpy(&d, &bits_or_val, 8);
            return topn_f64_ord(d);
        };
        uint64_t olo = 0, ohi = 0;
        bool any = false, full = false;
        uint32_t pl = 0;
        if (const cs_lookup *lk = cs_col_lookup(s, col, &pl)) {
            /* a derived column: the [min, max] of its payload array */
            olo = ord_i(lk->n ? lk->plo[pl] : 0);
            ohi = ord_i(lk->n ? lk->phi[pl] : 0);
        } else if (const cs_expr *ex = cs_col_expr(s, col)) {
            /* a computed column: the [min, max] its evaluation measured */
            olo = ord_i(ex->lo);
            ohi = ord_i(ex->hi);
        } else if (t == CSTRIPE_VARTEXT) {
            /* dictionary ranks: exactly [0, n_dict - 1] */
            const int64_t nd = (int64_t)s->text_dicts[col].offsets.size() - 1;
            olo = ord_i(0);
            ohi = ord_i(nd > 0 ? nd - 1 : 0);
        } else {
            for (const cs_selchunk &sc : s->sel) {
                const csf_skipnode &nd = r->stripes[sc.stripe].nodes[col][sc.chunk].n;
                if (nd.has_min_max) {
                    const uint64_t a = ord_node(nd.min_i), b = ord_node(nd.max_i);
                    if (!any) { olo = a; ohi = b; any = true; }
                    else { olo = std::min(olo, a); ohi = std::max(ohi, b); }
                } else if (nd.n_present > 0) {
                    full = true;
                }
            }
            if (full) {
                switch (t) {
                    case CSTRIPE_I8:  olo = ord_i(INT8_MIN);  ohi = ord_i(INT8_MAX);  break;
                    case CSTRIPE_I16: olo = ord_i(INT16_MIN); ohi = ord_i(INT16_MAX); break;
                    case CSTRIPE_I32: olo = ord_i(INT32_MIN); ohi = ord_i(INT32_MAX); break;
                    case CSTRIPE_I64: olo = ord_i(INT64_MIN); ohi = ord_i(INT64_MAX); break;
                    default:
                        olo = topn_f64_ord(-__builtin_inf());
                        ohi = topn_f64_ord(__builtin_nan(""));
                        break;
                }
            }
            if (ohi < olo) { olo = 0; ohi = 0; }
        }
        tp.klo[k] = olo;
        tp.kspan[k] = ohi - olo;
        kbits[k] = tp.kspan[k] == ~0ull ? 65u : hash_bitlen(tp.kspan[k] + 1);
        total_bits += kbits[k];
    }
    if (total_bits > 64) {
        char msg[160];
        int w = 0;
        for (uint32_t k = 0; k < n_order; k++)
            w += snprintf(msg + w, sizeof(msg) - (size_t)w, "%scol %u: %u bits",
                          k ? ", " : "", order[k].column, kbits[k]);
        cs_set_err("scan_select_topn: packed key needs %u bits > 64 (%s) — key ranges "
                   "come from the selected chunk groups' min/max", total_bits, msg);
        return CSTRIPE_ERR_ARG;
    }
    /* column 0 most significant */
    for (uint32_t k = n_order, sh = 0; k-- > 0;) {
        tp.kshift[k] = sh;
        sh += kbits[k];
    }

    AggParams p{};
    { int _rc = select_prepare(s, p); if (_rc != CSTRIPE_OK) return _rc; }
    sp.tiles_per_group = p.tiles_per_group;
    tp.tiles_per_group = p.tiles_per_group;
    if (g->n_groups == 0) {
        topn_zero_timing(s);
        out->n_rows = 0;
        return CSTRIPE_OK;
    }
    for (hipEvent_t &e : g->tev)
        if (!e) HIP_TRY(hipEventCreate(&e));

    float ms_d = 0, ms_m = 0, ms_o = 0;
    bool decoded = false;
    if (!g->sel_cached) {
        { int _rc = select_run_count(s, p); if (_rc != CSTRIPE_OK) return _rc; }
        ms_d = (float)s->last_decode_ms;
        ms_m = (float)s->last_select_mask_ms;
        ms_o = (float)s->last_select_offsets_ms;
        decoded = true;     /* same stream, nothing in between */
    }
    const uint64_t n_pass = g->sel_total;
    s->last_select_mask_ms = ms_m;
    s->last_select_offsets_ms = ms_o;
    s->last_select_emit_ms = 0;
    s->last_agg_ms = 0;
    if (n_pass == 0) {
        s->last_decode_ms = ms_d;
        s->last_kernel_ms = ms_d + ms_m + ms_o;
        s->last_topn_key_ms = s->last_topn_select_ms = s->last_topn_emit_ms = 0;
        out->n_rows = 0;
        return CSTRIPE_OK;
    }
    const uint64_t m = std::min<uint64_t>(limit, n_pass);
    const bool selecting = n_pass > limit;
    const uint32_t n_tiles = g->n_groups * p.tiles_per_group;
    tp.n_keys = n_pass;

    /* scan-order rows (emit) and, in host mode, the permuted staging */
    uint64_t off_vals[MAX_PROJ], off_nulls[MAX_PROJ], off_rn = 0, need = 0;
    bool want_nulls[MAX_PROJ];
    for (uint32_t i = 0; i < sp.n_cols; i++) {
        want_nulls[i] = out->col_nulls && out->col_nulls[dst_col[i]];
        off_vals[i] = need;
        need = align_up(need + m * widths[i], 16);
        off_nulls[i] = need;
        if (want_nulls[i]) need = align_up(need + m, 16);
    }
    off_rn = need;
    if (out->row_numbers) need += m * sizeof(uint64_t);
    if (need == 0) need = 16;

    { int _rc = hash_grow(g->d_tn_keys, g->tn_keys_n, n_pass); if (_rc != CSTRIPE_OK) return _rc; }
    { int _rc = hash_grow(g->d_tn_emit, g->tn_emit_bytes, need); if (_rc != CSTRIPE_OK) return _rc; }
    { int _rc = hash_grow(g->d_tn_perm, g->tn_perm_n, m); if (_rc != CSTRIPE_OK) return _rc; }
    if (!dst_on_device) { int _rc = hash_grow(g->d_tn_out, g->tn_out_bytes, need); if (_rc != CSTRIPE_OK) return _rc; }
    if (selecting) {
        const uint64_t words = (uint64_t)n_tiles * SEL_SLICES;
        { int _rc = hash_grow(g->d_tn_okeys, g->tn_okeys_n, m); if (_rc != CSTRIPE_OK) return _rc; }
        { int _rc = hash_grow(g->d_tn_mask, g->tn_mask_n, words); if (_rc != CSTRIPE_OK) return _rc; }
        { int _rc = hash_grow(g->d_tn_eq, g->tn_eq_n, words); if (_rc != CSTRIPE_OK) return _rc; }
        { int _rc = hash_grow(g->d_tn_counts, g->tn_counts_n, (uint64_t)n_tiles); if (_rc != CSTRIPE_OK) return _rc; }
        { int _rc = hash_grow(g->d_tn_tbases, g->tn_tbases_n, (uint64_t)n_tiles); if (_rc != CSTRIPE_OK) return _rc; }
        { int _rc = hash_grow(g->d_tn_bases, g->tn_bases_n, (uint64_t)n_tiles); if (_rc != CSTRIPE_OK) return _rc; }
        if (!g->d_tn_state) HIP_TRY(hipMalloc(&g->d_tn_state, sizeof(TopnState)));
        if (!g->d_tn_total) HIP_TRY(hipMalloc(&g->d_tn_total, 2 * sizeof(uint64_t)));
    }

    HIP_TRY(hipMemsetAsync(g->d_error, 0, sizeof(int), g->stream));
    HIP_TRY(hipEventRecord(g->tev[0], g->stream));
    if (!decoded) { int _rc = launch_decode(g); if (_rc != CSTRIPE_OK) return _rc; }
    HIP_TRY(hipEventRecord(g->tev[1], g->stream));
    hipLaunchKernelGGL(topn_key_kernel, dim3(n_tiles), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_data, g->d_scratch, g->d_rank, g->d_groups, g->d_colloc,
                       g->d_sel_mask, g->d_sel_bases, g->d_tn_keys, g->d_error, tp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->tev[2], g->stream));
    if (selecting) {
        const uint32_t rounds = (total_bits + 7) / 8;       /* 1..8 */
        const uint64_t kblocks = (n_pass + AGG_BLOCK - 1) / AGG_BLOCK;
        const uint32_t hgrid = (uint32_t)std::min<uint64_t>(kblocks, TOPN_GRID);
        hipLaunchKernelGGL(topn_init_kernel, dim3(1), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_tn_state, limit);
        for (uint32_t rd = 0; rd < rounds; rd++) {
            const uint32_t shift = 8 * (rounds - 1 - rd);
            hipLaunchKernelGGL(topn_hist_kernel, dim3(hgrid), dim3(AGG_BLOCK), 0, g->stream,
                               g->d_tn_keys, n_pass, g->d_tn_state, shift);
            hipLaunchKernelGGL(topn_pick_kernel, dim3(1), dim3(WAVE), 0, g->stream,
                               g->d_tn_state);
        }
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(topn_refine_kernel, dim3(n_tiles), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_sel_mask, g->d_sel_bases, g->d_tn_keys, n_pass,
                           g->d_tn_state, g->d_tn_mask, g->d_tn_eq, g->d_tn_counts);
        hipLaunchKernelGGL(select_offsets_kernel, dim3(1), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_tn_counts, g->d_tn_tbases, g->d_tn_total, n_tiles);
        hipLaunchKernelGGL(topn_final_kernel, dim3(n_tiles), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_tn_eq, g->d_tn_tbases, g->d_tn_state, g->d_tn_mask,
                           g->d_tn_counts);
        hipLaunchKernelGGL(select_offsets_kernel, dim3(1), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_tn_counts, g->d_tn_bases, g->d_tn_total + 1, n_tiles);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(g->tev[3], g->stream));

    /* one sync before anything is emitted: the range flag, and the refined
     * total, which must be exactly `limit` — the emit buffers are sized by it */
    int h_err = 0;
    uint64_t h_tot[2] = {0, m};
    HIP_TRY(hipMemcpyAsync(&h_err, g->d_error, sizeof(int), hipMemcpyDeviceToHost, g->stream));
    if (selecting)
        HIP_TRY(hipMemcpyAsync(h_tot, g->d_tn_total, sizeof(h_tot), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (h_err & TOPN_ERR_RANGE) {
        cs_set_err("scan_select_topn: an order value lies outside its chunk's recorded min/max "
                   "(device flag %d) — corrupt skip nodes", h_err);
        return CSTRIPE_ERR_FORMAT;
    }
    if (h_err) { cs_set_err("decode error on device (flag %d)", h_err); return CSTRIPE_ERR_FORMAT; }
    if (h_tot[1] != m) {
        cs_set_err("scan_select_topn: selection kept %llu rows, expected %llu",
                   (unsigned long long)h_tot[1], (unsigned long long)m);
        return CSTRIPE_ERR;
    }

    for (uint32_t i = 0; i < sp.n_cols; i++) {
        sp.cols[i].vals = g->d_tn_emit + off_vals[i];
        sp.cols[i].nulls = want_nulls[i] ? g->d_tn_emit + off_nulls[i] : nullptr;
    }
    sp.row_numbers = out->row_numbers ? (uint64_t *)(g->d_tn_emit + off_rn) : nullptr;
    HIP_TRY(hipEventRecord(g->tev[4], g->stream));
    hipLaunchKernelGGL(select_emit_kernel, dim3(n_tiles), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_data, g->d_scratch, g->d_rank, g->d_groups, g->d_colloc,
                       selecting ? g->d_tn_mask : g->d_sel_mask,
                       selecting ? g->d_tn_bases : g->d_sel_bases, g->d_sel_rowbase, sp);
    if (selecting)
        hipLaunchKernelGGL(topn_keygather_kernel, dim3(n_tiles), dim3(AGG_BLOCK), 0, g->stream,
                           g->d_sel_mask, g->d_sel_bases, g->d_tn_mask, g->d_tn_bases,
                           g->d_tn_keys, n_pass, g->d_tn_okeys, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->tev[5], g->stream));

    /* the m (key, ordinal) pairs: ordinals are scan order, so a stable sort
     * by key is the sort by (key, row number) */
    std::vector<uint64_t> h_keys(m);
    HIP_TRY(hipMemcpyAsync(h_keys.data(), selecting ? g->d_tn_okeys : g->d_tn_keys,
                           m * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    std::vector<uint32_t> h_perm(m);
    for (uint64_t i = 0; i < m; i++) h_perm[i] = (uint32_t)i;
    std::stable_sort(h_perm.begin(), h_perm.end(),
                     [&](uint32_t a, uint32_t b) { return h_keys[a] < h_keys[b]; });
    HIP_TRY(hipMemcpyAsync(g->d_tn_perm, h_perm.data(), m * sizeof(uint32_t),
                           hipMemcpyHostToDevice, g->stream));

    PermParams pp{};
    pp.n_cols = sp.n_cols;
    pp.n = m;
    for (uint32_t i = 0; i < sp.n_cols; i++) {
        PermCol &pc = pp.cols[i];
        pc.width = widths[i];
        pc.src_vals = sp.cols[i].vals;
        pc.src_nulls = sp.cols[i].nulls;
        if (dst_on_device) {
            pc.dst_vals = (uint8_t *)out->col_values[dst_col[i]];
            pc.dst_nulls = want_nulls[i] ? out->col_nulls[dst_col[i]] : nullptr;
        } else {
            pc.dst_vals = g->d_tn_out + off_vals[i];
            pc.dst_nulls = want_nulls[i] ? g->d_tn_out + off_nulls[i] : nullptr;
        }
    }
    pp.src_rn = sp.row_numbers;
    pp.dst_rn = !out->row_numbers ? nullptr
              : dst_on_device ? out->row_numbers : (uint64_t *)(g->d_tn_out + off_rn);
    const uint32_t pgrid = (uint32_t)std::min<uint64_t>((m + AGG_BLOCK - 1) / AGG_BLOCK, TOPN_GRID);
    HIP_TRY(hipEventRecord(g->tev[6], g->stream));
    hipLaunchKernelGGL(topn_permute_kernel, dim3(pgrid), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_tn_perm, pp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->tev[7], g->stream));
    if (!dst_on_device) {
        for (uint32_t i = 0; i < sp.n_cols; i++) {
            HIP_TRY(hipMemcpyAsync(out->col_values[dst_col[i]], pp.cols[i].dst_vals,
                                   m * widths[i], hipMemcpyDeviceToHost, g->stream));
            if (want_nulls[i])
                HIP_TRY(hipMemcpyAsync(out->col_nulls[dst_col[i]], pp.cols[i].dst_nulls,
                                       m, hipMemcpyDeviceToHost, g->stream));
        }
        if (pp.dst_rn)
            HIP_TRY(hipMemcpyAsync(out->row_numbers, pp.dst_rn, m * sizeof(uint64_t),
                                   hipMemcpyDeviceToHost, g->stream));
    }
    HIP_TRY(hipStreamSynchronize(g->stream));   /* h_perm leaves scope */

    float ms_d2 = 0, ms_k = 0, ms_s = 0, ms_e = 0, ms_p = 0;
    (void)hipEventElapsedTime(&ms_d2, g->tev[0], g->tev[1]);
    (void)hipEventElapsedTime(&ms_k, g->tev[1], g->tev[2]);
    (void)hipEventElapsedTime(&ms_s, g->tev[2], g->tev[3]);
    (void)hipEventElapsedTime(&ms_e, g->tev[4], g->tev[5]);
    (void)hipEventElapsedTime(&ms_p, g->tev[6], g->tev[7]);
    s->last_decode_ms = ms_d + ms_d2;
    s->last_topn_key_ms = ms_k;
    if (!selecting) ms_s = 0;           /* nothing ran between the two events */
    s->last_topn_select_ms = ms_s;
    s->last_topn_emit_ms = ms_e + ms_p;
    s->last_kernel_ms = ms_d + ms_d2 + ms_m + ms_o + ms_k + ms_s + ms_e + ms_p;
    out->n_rows = m;
    return CSTRIPE_OK;
}

/* =====================================================================
 * scan_agg_hashed_topn — GROUP BY ... [HAVING] ORDER BY ... LIMIT on the
 * device: what WorkerLimitCount / WorkerSortClauseList and
 * ProcessHavingClauseForWorkerQuery push to a worker whose groups are
 * disjoint from every other shard's (multi_logical_optimizer.c:5039-5212,
 * :2650-2682). Nothing new runs per row: after the front half of
 * scan_agg_hashed the `n` compacted groups sit in d_hokeys / d_hocells, and
 * on the scan's stream
 *
 *   gtopn_init_kernel     clears the state block
 *   gtopn_range_kernel    per group: the HAVING atoms; kept groups append
 *                         their index through one counter (wave-aggregated
 *                         add, as hash_compact_kernel); per AGG order term
 *                         the min / max order code over kept non-NULL groups
 *                         (block reduction, one atomicMin / atomicMax per
 *                         block); a flag per term for an integer sum outside
 *                         int64. The state block's copy-back is the one sync
 *                         before the selection; the host derives bits and
 *                         shifts from it.
 *   gtopn_key_kernel      per kept group the ORDER word (terms packed as
 *                         topn_key_kernel packs columns: offset from lo,
 *                         reversed for DESC, one NULL code at either end) and
 *                         the TIE word (the key tuple re-packed in output
 *                         order: column 0 most significant, NULL last)
 *   radix select          topn_init / topn_hist / topn_pick, unchanged, over
 *                         the order words: T1 and the number still wanted
 *                         among the groups on T1; then gtopn_tieinit_kernel +
 *                         gtopn_tiehist_kernel / topn_pick_kernel over the
 *                         tie words of exactly those groups: T2. Tie words
 *                         are distinct (one per key tuple), so
 *                         ord < T1 | (ord == T1 & tie <= T2) holds for
 *                         exactly `limit` groups. Skipped when kept <= limit.
 *   gtopn_gather_kernel   the selected groups' packed key, order word, tie
 *                         word and cells into limit-sized arrays
 *   (host)                one DtoH copy, a sort by (order word, tie word),
 *                         unpack, cell_to_partial
 *
 * No flag, fence, spin-wait or cross-block dependency exists inside a
 * kernel; kernel boundaries order the stages. Words several blocks touch —
 * the two counters, the range words, the overflow flags, the histogram bins —
 * are updated by integer atomics (add / min / max / or) alone; the append
 * positions the counters hand out depend on arrival order, the SET of
 * appended groups and every value derived from it do not, and the host sort
 * fixes the output order. Every loop is bounded by a count or a constant.
 * ===================================================================== */

#define GTOPN_GRID   1024
#define GT_CNT  0u      /* COUNT kinds: the count, never NULL */
#define GT_I64  1u      /* MIN / MAX_I64: the value in lo */
#define GT_I128 2u      /* integer sums */
#define GT_F64  3u

struct GtopnParams {
    uint32_t n_aggs, n_key_cols, n_having, n_order;
    uint32_t hagg[CSTRIPE_MAX_HAVING], hop[CSTRIPE_MAX_HAVING], hcls[CSTRIPE_MAX_HAVING];
    int64_t  hival[CSTRIPE_MAX_HAVING];
    uint64_t hford[CSTRIPE_MAX_HAVING];                 /* topn_f64_ord(fval) */
    uint32_t okind[CSTRIPE_MAX_GROUP_ORDER], oindex[CSTRIPE_MAX_GROUP_ORDER];
    uint32_t oflags[CSTRIPE_MAX_GROUP_ORDER], ocls[CSTRIPE_MAX_GROUP_ORDER];
    uint32_t oshift[CSTRIPE_MAX_GROUP_ORDER];
    uint64_t olo[CSTRIPE_MAX_GROUP_ORDER], ospan[CSTRIPE_MAX_GROUP_ORDER];
    uint32_t kshift[CSTRIPE_MAX_HASH_KEY_COLS], kbits[CSTRIPE_MAX_HASH_KEY_COLS];
    uint32_t tshift[CSTRIPE_MAX_HASH_KEY_COLS];         /* tie word */
    uint64_t kspan[CSTRIPE_MAX_HASH_KEY_COLS];
};

struct GtopnState {
    unsigned long long n_kept;          /* groups HAVING kept */
    unsigned long long n_out;           /* groups gathered */
    unsigned long long lo[CSTRIPE_MAX_GROUP_ORDER];   /* order codes, AGG terms */
    unsigned long long hi[CSTRIPE_MAX_GROUP_ORDER];
    unsigned int ovf;                   /* bit t: term t met a sum outside int64 */
    unsigned int pad;
};

static uint32_t gtopn_class(uint32_t kind)
{
    switch (kind) {
        case CSTRIPE_AGG_COUNT_STAR: case CSTRIPE_AGG_COUNT_COL: return GT_CNT;
        case CSTRIPE_AGG_MIN_I64: case CSTRIPE_AGG_MAX_I64: return GT_I64;
        case CSTRIPE_AGG_SUM_F64: case CSTRIPE_AGG_MIN_F64: case CSTRIPE_AGG_MAX_F64: return GT_F64;
        default: return GT_I128;
    }
}

__host__ __device__ inline bool gtopn_null(const AccCell &c, uint32_t cls)
{
    return cls != GT_CNT && c.cnt == 0;
}

/* order code of a non-NULL aggregate value: signed integers flip the sign
 * bit, floats go through topn_f64_ord; *ovf when an int128 sum is no int64 */
__host__ __device__ inline uint64_t gtopn_ord(const AccCell &c, uint32_t cls, bool *ovf)
{
    *ovf = false;
    if (cls == GT_CNT) return (uint64_t)c.cnt ^ TOPN_SIGN;
    if (cls == GT_F64) return topn_f64_ord(c.f);
    if (cls == GT_I128 && c.hi != (c.lo < 0 ? -1 : 0)) *ovf = true;
    return (uint64_t)c.lo ^ TOPN_SIGN;
}

/* one HAVING atom on the aggregate's final value; a NULL aggregate fails */
__device__ inline bool gtopn_having(const AccCell &c, uint32_t cls, uint32_t op,
                                    int64_t ival, uint64_t ford)
{
    int cmp;
    if (cls == GT_CNT) {
        cmp = c.cnt < ival ? -1 : (c.cnt > ival ? 1 : 0);
    } else {
        if (c.cnt == 0) return false;
        if (cls == GT_I64) {
            cmp = c.lo < ival ? -1 : (c.lo > ival ? 1 : 0);
        } else if (cls == GT_I128) {
            /* the full int128 against the sign-extended constant */
            const int64_t ihi = ival < 0 ? -1 : 0;
            if (c.hi != ihi) cmp = c.hi < ihi ? -1 : 1;
            else cmp = (uint64_t)c.lo < (uint64_t)ival ? -1
                     : ((uint64_t)c.lo > (uint64_t)ival ? 1 : 0);
        } else {
            const uint64_t o = topn_f64_ord(c.f);
            cmp = o < ford ? -1 : (o > ford ? 1 : 0);
        }
    }
    switch (op) {
        case CSTRIPE_PRED_LT: return cmp < 0;
        case CSTRIPE_PRED_LE: return cmp <= 0;
        case CSTRIPE_PRED_GT: return cmp > 0;
        case CSTRIPE_PRED_GE: return cmp >= 0;
        case CSTRIPE_PRED_EQ: return cmp == 0;
        default:              return cmp != 0;
    }
}

__device__ inline uint64_t gtopn_keycode(uint64_t key, const GtopnParams &gp, uint32_t k)
{
    return (key >> gp.kshift[k]) & ((1ull << gp.kbits[k]) - 1ull);   /* kbits <= 63 */
}

__global__ __launch_bounds__(WAVE) void gtopn_init_kernel(GtopnState *st)
{
    if (threadIdx.x == 0) { st->n_kept = 0; st->n_out = 0; st->ovf = 0; st->pad = 0; }
    if (threadIdx.x < CSTRIPE_MAX_GROUP_ORDER) {
        st->lo[threadIdx.x] = ~0ull;
        st->hi[threadIdx.x] = 0;
    }
}

__global__ __launch_bounds__(AGG_BLOCK) void gtopn_range_kernel(
    const AccCell *__restrict__ cells, uint64_t n, uint32_t *__restrict__ kept,
    GtopnState *st, const GtopnParams gp)
{
    __shared__ unsigned long long s_lo[CSTRIPE_MAX_GROUP_ORDER][AGG_BLOCK / WAVE];
    __shared__ unsigned long long s_hi[CSTRIPE_MAX_GROUP_ORDER][AGG_BLOCK / WAVE];
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t wid = threadIdx.x / WAVE;
    unsigned long long lo[CSTRIPE_MAX_GROUP_ORDER], hi[CSTRIPE_MAX_GROUP_ORDER];
    #pragma unroll
    for (uint32_t t = 0; t < CSTRIPE_MAX_GROUP_ORDER; t++) { lo[t] = ~0ull; hi[t] = 0; }
    unsigned int ovf = 0;
    /* wave-uniform trip count: the ballot below needs every lane present */
    for (uint64_t base = (uint64_t)blockIdx.x * AGG_BLOCK; base < n;
         base += (uint64_t)gridDim.x * AGG_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        bool keep = i < n;
        if (keep)
            for (uint32_t h = 0; h < gp.n_having; h++)
                keep = keep && gtopn_having(cells[i * gp.n_aggs + gp.hagg[h]], gp.hcls[h],
                                            gp.hop[h], gp.hival[h], gp.hford[h]);
        const uint64_t m = __ballot(keep);
        if (m == 0) continue;
        const int leader = __ffsll((unsigned long long)m) - 1;
        unsigned long long wbase = 0;
        if ((int)lane == leader)
            wbase = atomicAdd(&st->n_kept, (unsigned long long)__popcll(m));
        wbase = (unsigned long long)__shfl((long long)wbase, leader, WAVE);
        if (!keep) continue;
        /* every group is counted once, so the index stays below n */
        const uint64_t at = wbase + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
        if (at < n) kept[at] = (uint32_t)i;
        #pragma unroll
        for (uint32_t t = 0; t < CSTRIPE_MAX_GROUP_ORDER; t++) {
            if (t >= gp.n_order || gp.okind[t] != CSTRIPE_GORDER_AGG) continue;
            const AccCell c = cells[i * gp.n_aggs + gp.oindex[t]];
            if (gtopn_null(c, gp.ocls[t])) continue;
            bool of;
            const unsigned long long o = gtopn_ord(c, gp.ocls[t], &of);
            if (of) { ovf |= 1u << t; continue; }
            lo[t] = o < lo[t] ? o : lo[t];
            hi[t] = o > hi[t] ? o : hi[t];
        }
    }
    if (ovf) atomicOr(&st->ovf, ovf);
    #pragma unroll
    for (uint32_t t = 0; t < CSTRIPE_MAX_GROUP_ORDER; t++) {
        unsigned long long l = lo[t], h = hi[t];
        #pragma unroll
        for (int d = WAVE / 2; d > 0; d >>= 1) {
            const unsigned long long l2 = (unsigned long long)__shfl_xor((long long)l, d, WAVE);
            const unsigned long long h2 = (unsigned long long)__shfl_xor((long long)h, d, WAVE);
            l = l2 < l ? l2 : l;
            h = h2 > h ? h2 : h;
        }
        if (lane == 0) { s_lo[t][wid] = l; s_hi[t][wid] = h; }
    }
    __syncthreads();
    if (threadIdx.x < CSTRIPE_MAX_GROUP_ORDER) {
        const uint32_t t = threadIdx.x;
        unsigned long long l = ~0ull, h = 0;
        for (uint32_t w = 0; w < AGG_BLOCK / WAVE; w++) {
            l = s_lo[t][w] < l ? s_lo[t][w] : l;
            h = s_hi[t][w] > h ? s_hi[t][w] : h;
        }
        if (l <= h) {                   /* this block saw a value of term t */
            atomicMin(&st->lo[t], l);
            atomicMax(&st->hi[t], h);
        }
    }
}

__global__ __launch_bounds__(AGG_BLOCK) void gtopn_key_kernel(
    const unsigned long long *__restrict__ okeys, const AccCell *__restrict__ cells,
    const uint32_t *__restrict__ kept, uint64_t n_kept, uint64_t *__restrict__ ord,
    uint64_t *__restrict__ tie, const GtopnParams gp)
{
    for (uint64_t j = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; j < n_kept;
         j += (uint64_t)gridDim.x * AGG_BLOCK) {
        const uint64_t i = kept[j];
        const uint64_t key = okeys[i];
        uint64_t ow = 0;
        for (uint32_t t = 0; t < gp.n_order; t++) {
            const uint32_t fl = gp.oflags[t];
            const uint64_t span = gp.ospan[t];
            bool null;
            uint64_t d = 0;
            if (gp.okind[t] == CSTRIPE_GORDER_AGG) {
                const AccCell c = cells[i * gp.n_aggs + gp.oindex[t]];
                null = gtopn_null(c, gp.ocls[t]);
                if (!null) {
                    bool of;
                    d = gtopn_ord(c, gp.ocls[t], &of) - gp.olo[t];
                    if (d > span) d = span;     /* measured over these groups: never */
                }
            } else {
                const uint64_t kc = gtopn_keycode(key, gp, gp.oindex[t]);
                null = kc == 0;
                d = kc - 1;
            }
            uint64_t code;
            if (!null) {
                if (fl & CSTRIPE_ORDER_DESC) d = span - d;
                code = (fl & CSTRIPE_ORDER_NULLS_FIRST) ? d + 1 : d;
            } else {
                code = (fl & CSTRIPE_ORDER_NULLS_FIRST) ? 0 : span + 1;
            }
            ow |= code << gp.oshift[t];
        }
        uint64_t tw = 0;
        for (uint32_t k = 0; k < gp.n_key_cols; k++) {
            const uint64_t kc = gtopn_keycode(key, gp, k);
            tw |= (kc == 0 ? gp.kspan[k] + 1 : kc - 1) << gp.tshift[k];
        }
        ord[j] = ow;
        tie[j] = tw;
    }
}

/* the tie-word select starts where the order-word select ended: it wants
 * the st_ord->k smallest tie words among the groups on the threshold */
__global__ __launch_bounds__(AGG_BLOCK) void gtopn_tieinit_kernel(
    TopnState *st_tie, const TopnState *__restrict__ st_ord)
{
    st_tie->hist[threadIdx.x] = 0;      /* AGG_BLOCK == 256 bins */
    if (threadIdx.x == 0) { st_tie->prefix = 0; st_tie->k = st_ord->k; }
}

/* topn_hist_kernel over the tie words, restricted to the groups whose order
 * word equals the threshold */
__global__ __launch_bounds__(AGG_BLOCK) void gtopn_tiehist_kernel(
    const uint64_t *__restrict__ ord, const uint64_t *__restrict__ tie, uint64_t n,
    const TopnState *__restrict__ st_ord, TopnState *st_tie, uint32_t shift)
{
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t T1 = st_ord->prefix;
    const uint64_t prefix = st_tie->prefix;
    const bool top = shift + 8 >= 64;
    const uint32_t hs = top ? 0 : shift + 8;
    for (uint64_t i = (uint64_t)blockIdx.x * AGG_BLOCK + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * AGG_BLOCK) {
        if (ord[i] != T1) continue;
        const uint64_t key = tie[i];
        if (top || (key >> hs) == prefix)
            atomicAdd(&lh[(key >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    if (c) atomicAdd(&st_tie->hist[threadIdx.x], (unsigned long long)c);
}

/* out: [m] packed keys | [m] order words | [m] tie words | [m * n_aggs] cells */
__global__ __launch_bounds__(AGG_BLOCK) void gtopn_gather_kernel(
    const unsigned long long *__restrict__ okeys, const AccCell *__restrict__ cells,
    const uint32_t *__restrict__ kept, uint64_t n_kept,
    const uint64_t *__restrict__ ord, const uint64_t *__restrict__ tie,
    const TopnState *__restrict__ st_ord, const TopnState *__restrict__ st_tie,
    int all, GtopnState *st, uint64_t m, uint8_t *__restrict__ outb, uint32_t n_aggs)
{
    const uint32_t lane = threadIdx.x % WAVE;
    const uint64_t T1 = all ? 0 : st_ord->prefix;
    const uint64_t T2 = all ? 0 : st_tie->prefix;
    uint64_t *o_key = (uint64_t *)outb;
    uint64_t *o_ord = o_key + m;
    uint64_t *o_tie = o_ord + m;
    AccCell *o_cells = (AccCell *)(o_tie + m);
    /* wave-uniform trip count: the ballot below needs every lane present */
    for (uint64_t base = (uint64_t)blockIdx.x * AGG_BLOCK; base < n_kept;
         base += (uint64_t)gridDim.x * AGG_BLOCK) {
        const uint64_t j = base + threadIdx.x;
        bool take = false;
        uint64_t ow = 0, tw = 0;
        if (j < n_kept) {
            ow = ord[j];
            tw = tie[j];
            take = all || ow < T1 || (ow == T1 && tw <= T2);
        }
        const uint64_t mk = __ballot(take);
        if (mk == 0) continue;
        const int leader = __ffsll((unsigned long long)mk) - 1;
        unsigned long long wbase = 0;
        if ((int)lane == leader)
            wbase = atomicAdd(&st->n_out, (unsigned long long)__popcll(mk));
        wbase = (unsigned long long)__shfl((long long)wbase, leader, WAVE);
        if (!take) continue;
        /* the count stays exact (the host checks it); writes are bounded */
        const uint64_t at = wbase + (uint64_t)__popcll(mk & ((1ull << lane) - 1ull));
        if (at >= m) continue;
        const uint64_t i = kept[j];
        o_key[at] = okeys[i];
        o_ord[at] = ow;
        o_tie[at] = tw;
        for (uint32_t a = 0; a < n_aggs; a++)
            o_cells[at * n_aggs + a] = cells[i * n_aggs + a];
    }
}

int csgpu_agg_hashed_topn(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                          const uint32_t *key_cols, uint32_t n_key_cols,
                          uint64_t capacity, const cstripe_having *having,
                          uint32_t n_having, const cstripe_group_order *order,
                          uint32_t n_order, uint64_t limit, cstripe_hgroups *out)
{
    if (!s->gpu) { cs_set_err("scan not staged — call cstripe_gpu_stage first (GPU required; no CPU fallback)"); return CSTRIPE_ERR_NOGPU; }
    cs_gpu_state *g = s->gpu;
    if (limit == 0 || limit > CSTRIPE_MAX_TOPN) {
        cs_set_err("scan_agg_hashed_topn: limit %llu outside 1..%u",
                   (unsigned long long)limit, CSTRIPE_MAX_TOPN);
        return CSTRIPE_ERR_ARG;
    }
    if (n_order > CSTRIPE_MAX_GROUP_ORDER || (n_order && !order)) {
        cs_set_err("scan_agg_hashed_topn: %u order terms (0..%d)", n_order, CSTRIPE_MAX_GROUP_ORDER);
        return CSTRIPE_ERR_ARG;
    }
    if (n_having > CSTRIPE_MAX_HAVING || (n_having && !having)) {
        cs_set_err("scan_agg_hashed_topn: %u HAVING atoms (0..%d)", n_having, CSTRIPE_MAX_HAVING);
        return CSTRIPE_ERR_ARG;
    }
    HashFront hf;
    { int _rc = hash_prepare(s, aggs, n_aggs, key_cols, n_key_cols, capacity, out, hf); if (_rc != CSTRIPE_OK) return _rc; }
    const HashParams &hp = hf.hp;

    GtopnParams gp{};
    gp.n_aggs = n_aggs;
    gp.n_key_cols = n_key_cols;
    gp.n_having = n_having;
    gp.n_order = n_order;
    for (uint32_t h = 0; h < n_having; h++) {
        if (having[h].agg >= n_aggs) {
            cs_set_err("scan_agg_hashed_topn: HAVING atom %u: agg %u out of range (%u aggs)",
                       h, having[h].agg, n_aggs);
            return CSTRIPE_ERR_ARG;
        }
        if (having[h].op > CSTRIPE_PRED_NE) {
            cs_set_err("scan_agg_hashed_topn: HAVING atom %u: bad op %u (LT..NE)", h, having[h].op);
            return CSTRIPE_ERR_ARG;
        }
        gp.hagg[h] = having[h].agg;
        gp.hop[h] = having[h].op;
        gp.hcls[h] = gtopn_class(aggs[having[h].agg].kind);
        gp.hival[h] = having[h].ival;
        gp.hford[h] = topn_f64_ord(having[h].fval);
    }
    for (uint32_t t = 0; t < n_order; t++) {
        const cstripe_group_order &o = order[t];
        if (o.kind > CSTRIPE_GORDER_KEY) {
            cs_set_err("scan_agg_hashed_topn: order term %u: bad kind %u", t, o.kind);
            return CSTRIPE_ERR_ARG;
        }
        const bool is_key = o.kind == CSTRIPE_GORDER_KEY;
        if (o.index >= (is_key ? n_key_cols : n_aggs)) {
            cs_set_err("scan_agg_hashed_topn: order term %u: %s index %u out of range", t,
                       is_key ? "key" : "agg", o.index);
            return CSTRIPE_ERR_ARG;
        }
        if (o.flags & ~(CSTRIPE_ORDER_DESC | CSTRIPE_ORDER_NULLS_FIRST)) {
            cs_set_err("scan_agg_hashed_topn: order term %u: unknown flags 0x%x", t, o.flags);
            return CSTRIPE_ERR_ARG;
        }
        for (uint32_t j = 0; j < t; j++)
            if (order[j].kind == o.kind && order[j].index == o.index) {
                cs_set_err("scan_agg_hashed_topn: order term %u repeats term %u", t, j);
                return CSTRIPE_ERR_ARG;
            }
        if (is_key && cs_col_type(s, key_cols[o.index]) == CSTRIPE_TEXT) {
            cs_set_err("scan_select_topn: order col %u is TEXT — its row-level order in this "
                       "ABI is whole-slot, not collation; order by a VARTEXT column instead",
                       key_cols[o.index]);
            return CSTRIPE_ERR_ARG;
        }
        gp.okind[t] = o.kind;
        gp.oindex[t] = o.index;
        gp.oflags[t] = o.flags;
        gp.ocls[t] = is_key ? 0 : gtopn_class(aggs[o.index].kind);
    }
    uint32_t tie_bits = 0;
    for (uint32_t k = 0; k < n_key_cols; k++) {
        if (hp.klex[k]) {
            cs_set_err("scan_agg_hashed_topn: the key tuple only packs through the TEXT "
                       "order-key fallback, whose packed order is not the output order — "
                       "use cstripe_scan_agg_hashed");
            return CSTRIPE_ERR_ARG;
        }
        gp.kshift[k] = hp.kshift[k];
        gp.kbits[k] = hf.kbits[k];
        gp.kspan[k] = hp.kspan[k];
        tie_bits += hf.kbits[k];
    }
    /* tie word: column 0 most significant; same widths, so <= 63 bits */
    for (uint32_t k = 0, sh = tie_bits; k < n_key_cols; k++) {
        sh -= hf.kbits[k];
        gp.tshift[k] = sh;
    }

    s->last_gt_groups = s->last_gt_kept = 0;
    s->last_gt_range_ms = s->last_gt_select_ms = s->last_gt_emit_ms = 0;
    { int _rc = hash_execute(s, n_aggs, capacity, hf); if (_rc != CSTRIPE_OK) return _rc; }
    const uint64_t n = hf.n;
    s->last_gt_groups = n;
    if (n == 0) { out->n_groups = 0; return CSTRIPE_OK; }

    for (hipEvent_t &e : g->gev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    { int _rc = hash_grow(g->d_gt_kept, g->gt_kept_n, capacity); if (_rc != CSTRIPE_OK) return _rc; }
    { int _rc = hash_grow(g->d_gt_ord, g->gt_ord_n, capacity); if (_rc != CSTRIPE_OK) return _rc; }
    { int _rc = hash_grow(g->d_gt_tie, g->gt_tie_n, capacity); if (_rc != CSTRIPE_OK) return _rc; }
    if (!g->d_gt_state) HIP_TRY(hipMalloc(&g->d_gt_state, sizeof(GtopnState)));
    if (!g->d_gt_sel) HIP_TRY(hipMalloc(&g->d_gt_sel, 2 * sizeof(TopnState)));

    const uint32_t ngrid = (uint32_t)std::min<uint64_t>((n + AGG_BLOCK - 1) / AGG_BLOCK, GTOPN_GRID);
    HIP_TRY(hipEventRecord(g->gev[0], g->stream));
    hipLaunchKernelGGL(gtopn_init_kernel, dim3(1), dim3(WAVE), 0, g->stream, g->d_gt_state);
    hipLaunchKernelGGL(gtopn_range_kernel, dim3(ngrid), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_hocells, n, g->d_gt_kept, g->d_gt_state, gp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->gev[1], g->stream));

    /* the state block: the single sync before the selection */
    GtopnState h_st{};
    HIP_TRY(hipMemcpyAsync(&h_st, g->d_gt_state, sizeof(h_st), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    float ms_r = 0;
    (void)hipEventElapsedTime(&ms_r, g->gev[0], g->gev[1]);
    s->last_gt_range_ms = ms_r;
    s->last_kernel_ms += ms_r;
    const uint64_t n_kept = h_st.n_kept;
    s->last_gt_kept = n_kept;
    if (n_kept > n) {
        cs_set_err("scan_agg_hashed_topn: HAVING kept %llu of %llu groups",
                   (unsigned long long)n_kept, (unsigned long long)n);
        return CSTRIPE_ERR;
    }
    for (uint32_t t = 0; t < n_order; t++)
        if (h_st.ovf & (1u << t)) {
            cs_set_err("scan_agg_hashed_topn: order term %u: agg %u (kind %u) has a sum outside "
                       "int64 in a surviving group — such a value does not fit the 64-bit order "
                       "word", t, gp.oindex[t], aggs[gp.oindex[t]].kind);
            return CSTRIPE_ERR_ARG;
        }
    if (n_kept == 0) { out->n_groups = 0; return CSTRIPE_OK; }

    /* bits and shifts of the order word, term 0 most significant */
    uint32_t obits[CSTRIPE_MAX_GROUP_ORDER] = {0};
    uint32_t order_bits = 0;
    for (uint32_t t = 0; t < n_order; t++) {
        if (gp.okind[t] == CSTRIPE_GORDER_AGG) {
            const bool any = h_st.lo[t] <= h_st.hi[t];      /* a non-NULL value */
            gp.olo[t] = any ? h_st.lo[t] : 0;
            gp.ospan[t] = any ? h_st.hi[t] - h_st.lo[t] : 0;
        } else {
            gp.olo[t] = 0;
            gp.ospan[t] = hp.kspan[gp.oindex[t]];
        }
        obits[t] = gp.ospan[t] == ~0ull ? 65u : hash_bitlen(gp.ospan[t] + 1);
        order_bits += obits[t];
    }
    if (order_bits > 64) {
        char msg[200];
        int w = 0;
        for (uint32_t t = 0; t < n_order; t++)
            w += snprintf(msg + w, sizeof(msg) - (size_t)w, "%sterm %u (%s %u): %u bits",
                          t ? ", " : "", t,
                          gp.okind[t] == CSTRIPE_GORDER_KEY ? "key" : "agg", gp.oindex[t], obits[t]);
        cs_set_err("scan_agg_hashed_topn: order word needs %u bits > 64 (%s) — an aggregate "
                   "term's range is measured over the surviving groups, a key term's comes "
                   "from the key packing", order_bits, msg);
        return CSTRIPE_ERR_ARG;
    }
    for (uint32_t t = 0, sh = order_bits; t < n_order; t++) {
        sh -= obits[t];
        gp.oshift[t] = sh;
    }

    const uint64_t m = std::min<uint64_t>(limit, n_kept);
    const bool selecting = n_kept > limit;
    const uint64_t out_bytes = m * (3 * sizeof(uint64_t) + (uint64_t)n_aggs * sizeof(AccCell));
    { int _rc = hash_grow(g->d_gt_out, g->gt_out_bytes, out_bytes); if (_rc != CSTRIPE_OK) return _rc; }
    TopnState *st_ord = g->d_gt_sel, *st_tie = g->d_gt_sel + 1;
    const uint32_t kgrid = (uint32_t)std::min<uint64_t>((n_kept + AGG_BLOCK - 1) / AGG_BLOCK, GTOPN_GRID);

    HIP_TRY(hipEventRecord(g->gev[2], g->stream));
    hipLaunchKernelGGL(gtopn_key_kernel, dim3(kgrid), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_hokeys, g->d_hocells, g->d_gt_kept, n_kept,
                       g->d_gt_ord, g->d_gt_tie, gp);
    HIP_TRY(hipGetLastError());
    if (selecting) {
        const uint32_t orounds = (order_bits + 7) / 8;      /* 0..8 */
        const uint32_t trounds = (tie_bits + 7) / 8;        /* 1..8 */
        hipLaunchKernelGGL(topn_init_kernel, dim3(1), dim3(AGG_BLOCK), 0, g->stream,
                           st_ord, limit);
        for (uint32_t rd = 0; rd < orounds; rd++) {
            const uint32_t shift = 8 * (orounds - 1 - rd);
            hipLaunchKernelGGL(topn_hist_kernel, dim3(kgrid), dim3(AGG_BLOCK), 0, g->stream,
                               g->d_gt_ord, n_kept, st_ord, shift);
            hipLaunchKernelGGL(topn_pick_kernel, dim3(1), dim3(WAVE), 0, g->stream, st_ord);
        }
        hipLaunchKernelGGL(gtopn_tieinit_kernel, dim3(1), dim3(AGG_BLOCK), 0, g->stream,
                           st_tie, st_ord);
        for (uint32_t rd = 0; rd < trounds; rd++) {
            const uint32_t shift = 8 * (trounds - 1 - rd);
            hipLaunchKernelGGL(gtopn_tiehist_kernel, dim3(kgrid), dim3(AGG_BLOCK), 0, g->stream,
                               g->d_gt_ord, g->d_gt_tie, n_kept, st_ord, st_tie, shift);
            hipLaunchKernelGGL(topn_pick_kernel, dim3(1), dim3(WAVE), 0, g->stream, st_tie);
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(g->gev[3], g->stream));
    hipLaunchKernelGGL(gtopn_gather_kernel, dim3(kgrid), dim3(AGG_BLOCK), 0, g->stream,
                       g->d_hokeys, g->d_hocells, g->d_gt_kept, n_kept, g->d_gt_ord,
                       g->d_gt_tie, st_ord, st_tie, selecting ? 0 : 1, g->d_gt_state, m,
                       g->d_gt_out, n_aggs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g->gev[4], g->stream));

    /* limit-sized: the one result copy */
    std::vector<uint64_t> h_out(out_bytes / sizeof(uint64_t));
    HIP_TRY(hipMemcpyAsync(&h_st, g->d_gt_state, sizeof(h_st), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(h_out.data(), g->d_gt_out, out_bytes, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    float ms_s = 0, ms_e = 0;
    (void)hipEventElapsedTime(&ms_s, g->gev[2], g->gev[3]);
    (void)hipEventElapsedTime(&ms_e, g->gev[3], g->gev[4]);
    s->last_gt_select_ms = ms_s;
    s->last_gt_emit_ms = ms_e;
    s->last_kernel_ms += ms_s + ms_e;
    if (h_st.n_out != m) {
        cs_set_err("scan_agg_hashed_topn: selection kept %llu groups, expected %llu",
                   (unsigned long long)h_st.n_out, (unsigned long long)m);
        return CSTRIPE_ERR;
    }

    const uint64_t *h_key = h_out.data(), *h_ord = h_key + m, *h_tie = h_ord + m;
    const AccCell *h_cells = (const AccCell *)(h_tie + m);
    std::vector<uint32_t> perm(m);
    for (uint64_t i = 0; i < m; i++) perm[i] = (uint32_t)i;
    std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
        if (h_ord[a] != h_ord[b]) return h_ord[a] < h_ord[b];
        return h_tie[a] < h_tie[b];
    });
    for (uint64_t oi = 0; oi < m; oi++) {
        const uint64_t i = perm[oi];
        for (uint32_t k = 0; k < n_key_cols; k++) {
            const uint64_t code = (h_key[i] >> hp.kshift[k]) & ((1ull << hf.kbits[k]) - 1ull);
            out->key_nulls[k][oi] = code == 0 ? 1 : 0;
            out->keys[k][oi] = code == 0 ? 0 : (int64_t)((uint64_t)hp.klo[k] + (code - 1));
        }
        for (uint32_t a = 0; a < n_aggs; a++)
            out->partials[(size_t)oi * n_aggs + a] =
                cell_to_partial(aggs[a].kind, h_cells[(size_t)i * n_aggs + a]);
    }
    out->n_groups = m;
    return CSTRIPE_OK;
}

/* =====================================================================
 * Device write path: compress one chunk's columns ON the
 * GPU. Stats kernel reduces min/max and the OR-of-XOR signature that
 * decides the canonical mode; the emit kernel then writes the canonical
 * P(L)/CONST stream with one lane per value (every byte position is
 * closed-form — the same property the read path exploits). Columns that
 * do not fit a canonical parse are copied back raw and compressed by the
 * host writer path (greedy LZ4 / zstd / pglz), so any data works.
 * Replaces, for HBM-resident data, the host serializer of
 * SerializeChunkData/CompressBuffer (columnar_writer.c:592-654,
 * columnar_compression.c:62-158); only compressed bytes cross PCIe.
 * ===================================================================== */

struct WStats {
    int64_t mn, mx;            /* int: values; float: f64 bit patterns */
    uint64_t xsig;             /* OR of (v ^ v0) over the chunk (width 8) */
};

template <typename T>
__global__ __launch_bounds__(AGG_BLOCK) void wstats_kernel(
    const T *__restrict__ v, uint32_t n, int is_float, WStats *__restrict__ out)
{
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t xs = 0;
    uint64_t v0 = 0;
    if (n) __builtin_memcpy(&v0, &v[0], sizeof(T) < 8 ? sizeof(T) : 8);
    double fmn = 0, fmx = 0;
    bool seen = false;
    int64_t imn = INT64_MAX, imx = INT64_MIN;
    for (uint32_t i = tid; i < n; i += gridDim.x * blockDim.x) {
        if (is_float) {
            double d;
            if (sizeof(T) == 4) { float f; __builtin_memcpy(&f, &v[i], 4); d = f; }
            else __builtin_memcpy(&d, &v[i], 8);
            if (!seen) { fmn = fmx = d; seen = true; }
            else {
                if (f64cmp_pg(d, fmn) < 0) fmn = d;
                if (f64cmp_pg(d, fmx) > 0) fmx = d;
            }
        } else {
            const int64_t x = (int64_t)v[i];
            imn = min(imn, x);
            imx = max(imx, x);
        }
        if (sizeof(T) == 8) {               /* canonical signature: BIT xor */
            uint64_t bits;
            __builtin_memcpy(&bits, &v[i], 8);
            xs |= bits ^ v0;
        }
    }
    /* wave + LDS + global-atomic reduce */
    __shared__ int64_t smn[AGG_BLOCK / WAVE], smx[AGG_BLOCK / WAVE];
    __shared__ uint64_t sxs[AGG_BLOCK / WAVE];
    __shared__ int sseen[AGG_BLOCK / WAVE];
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const int64_t omn = __shfl_down((long long)(is_float ? (int64_t)__double_as_longlong(fmn) : imn), d, WAVE);
        const int64_t omx = __shfl_down((long long)(is_float ? (int64_t)__double_as_longlong(fmx) : imx), d, WAVE);
        const uint64_t oxs = (uint64_t)__shfl_down((long long)xs, d, WAVE);
        const int osn = __shfl_down((int)seen, d, WAVE);
        if (is_float) {
            double a, b;
            a = __longlong_as_double((long long)omn);
            b = __longlong_as_double((long long)omx);
            if (osn) {
                if (!seen) { fmn = a; fmx = b; seen = true; }
                else {
                    if (f64cmp_pg(a, fmn) < 0) fmn = a;
                    if (f64cmp_pg(b, fmx) > 0) fmx = b;
                }
            }
        } else {
            imn = min(imn, omn);
            imx = max(imx, omx);
        }
        xs |= oxs;
    }
    const uint32_t wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) {
        smn[wid] = is_float ? (int64_t)__double_as_longlong(fmn) : imn;
        smx[wid] = is_float ? (int64_t)__double_as_longlong(fmx) : imx;
        sxs[wid] = xs;
        sseen[wid] = seen;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t bmn = smn[0], bmx = smx[0];
        uint64_t bxs = sxs[0];
        int bseen = sseen[0];
        for (uint32_t w2 = 1; w2 < AGG_BLOCK / WAVE; w2++) {
            if (is_float) {
                if (sseen[w2]) {
                    double a = __longlong_as_double((long long)smn[w2]);
                    double b = __longlong_as_double((long long)smx[w2]);
                    if (!bseen) { bmn = smn[w2]; bmx = smx[w2]; bseen = 1; }
                    else {
                        if (f64cmp_pg(a, __longlong_as_double((long long)bmn)) < 0) bmn = smn[w2];
                        if (f64cmp_pg(b, __longlong_as_double((long long)bmx)) > 0) bmx = smx[w2];
                    }
                }
            } else {
                bmn = min(bmn, smn[w2]);
                bmx = max(bmx, smx[w2]);
            }
            bxs |= sxs[w2];
        }
        /* per-block results merged with CAS loops on the single out cell */
        if (is_float) {
            unsigned long long *amn = (unsigned long long *)&out->mn;
            unsigned long long cur = *amn;
            while (bseen) {
                double c = __longlong_as_double((long long)cur);
                double nv = __longlong_as_double((long long)bmn);
                if (f64cmp_pg(nv, c) >= 0) break;
                unsigned long long prev = atomicCAS(amn, cur, (unsigned long long)bmn);
                if (prev == cur) break;
                cur = prev;
            }
            unsigned long long *amx = (unsigned long long *)&out->mx;
            cur = *amx;
            while (bseen) {
                double c = __longlong_as_double((long long)cur);
                double nv = __longlong_as_double((long long)bmx);
                if (f64cmp_pg(nv, c) <= 0) break;
                unsigned long long prev = atomicCAS(amx, cur, (unsigned long long)bmx);
                if (prev == cur) break;
                cur = prev;
            }
        } else {
            atomicMin((long long *)&out->mn, (long long)bmn);
            atomicMax((long long *)&out->mx, (long long)bmx);
        }
        atomicOr((unsigned long long *)&out->xsig, (unsigned long long)bxs);
    }
}

/* emit the canonical P(L) stream for one width-8 column chunk: lane j
 * writes its value's literal bytes plus the token/offset of the sequence
 * it opens — every byte position is the closed form of format.h */
__global__ __launch_bounds__(AGG_BLOCK) void wemit_p_kernel(
    const uint64_t *__restrict__ v, uint32_t n, uint32_t L,
    uint8_t *__restrict__ out)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t step = L + 3u;
    const uint8_t mtok = (uint8_t)(8u - L - 4u);
    const uint64_t val = v[j];
    if (j == 0) {
        out[0] = (uint8_t)(((8u + L) << 4) | mtok);
        #pragma unroll
        for (int b = 0; b < 8; b++) out[1 + b] = (uint8_t)(val >> (8 * b));
        /* S0's offset closes after v1's low bytes (lane 1 writes those) */
        out[9 + L] = 8;
        out[10 + L] = 0;
        return;
    }
    if (j == n - 1) {                       /* final: token + full literals */
        const uint32_t fpos = (11u + L) + (n - 3u) * step;
        out[fpos] = (uint8_t)(8u << 4);
        #pragma unroll
        for (int b = 0; b < 8; b++) out[fpos + 1 + b] = (uint8_t)(val >> (8 * b));
        return;
    }
    /* v_j low bytes: j==1 lives in S0's literals at 9; j>=2 at pos(j) with
     * its sequence header [token at pos-1] and trailing offset */
    if (j == 1) {
        for (uint32_t b = 0; b < L; b++) out[9 + b] = (uint8_t)(val >> (8 * b));
        return;
    }
    const uint32_t pos = j * step + (6u - L);
    out[pos - 1] = (uint8_t)((L << 4) | mtok);
    for (uint32_t b = 0; b < L; b++) out[pos + b] = (uint8_t)(val >> (8 * b));
    out[pos + L] = 8;                       /* every S_i carries its offset */
    out[pos + L + 1] = 0;
}

int csgpu_compress_chunk(const void *const *dev_vals, const uint8_t *types,
                         uint32_t n_cols, uint32_t rows, uint64_t row_offset,
                         std::vector<cs_dev_chunk_col> &out)
{
    if (!cstripe_gpu_available()) { cs_set_err("device write path requires a visible MI355X"); return CSTRIPE_ERR_NOGPU; }
    out.assign(n_cols, {});
    hipStream_t st;
    HIP_TRY(hipStreamCreate(&st));
    WStats *d_stats = nullptr;
    uint8_t *d_out = nullptr;
    size_t d_out_cap = 0;
    auto cleanup = [&]() {
        if (d_stats) (void)hipFree(d_stats);
        if (d_out) (void)hipFree(d_out);
        (void)hipStreamDestroy(st);
    };
    #define WTRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) { \
        cs_set_err("%s failed: %s", #x, hipGetErrorString(_e)); cleanup(); return CSTRIPE_ERR; } } while (0)
    WTRY(hipMalloc(&d_stats, sizeof(WStats)));

    for (uint32_t c = 0; c < n_cols; c++) {
        const uint32_t width = csf_type_width(types[c]);
        const bool is_float = types[c] == CSTRIPE_F32 || types[c] == CSTRIPE_F64;
        const uint8_t *dv = (const uint8_t *)dev_vals[c] + row_offset * width;
        cs_dev_chunk_col &oc = out[c];
        oc.has_min_max = rows > 0;

        WStats init;
        if (is_float) {
            const double dnan = 0.0 / 0.0, dninf = -1.0 / 0.0;
            memcpy(&init.mn, &dnan, 8);     /* PG MIN identity: NaN high */
            memcpy(&init.mx, &dninf, 8);
        } else {
            init.mn = INT64_MAX;
            init.mx = INT64_MIN;
        }
        init.xsig = 0;
        WTRY(hipMemcpyAsync(d_stats, &init, sizeof(init), hipMemcpyHostToDevice, st));
        const uint32_t grid = rows ? min((rows + AGG_BLOCK - 1) / AGG_BLOCK, 1024u) : 1;
        if (rows) {
            switch (width) {
                case 1: hipLaunchKernelGGL(wstats_kernel<int8_t>, dim3(grid), dim3(AGG_BLOCK), 0, st, (const int8_t *)dv, rows, is_float, d_stats); break;
                case 2: hipLaunchKernelGGL(wstats_kernel<int16_t>, dim3(grid), dim3(AGG_BLOCK), 0, st, (const int16_t *)dv, rows, is_float, d_stats); break;
                case 4: hipLaunchKernelGGL(wstats_kernel<int32_t>, dim3(grid), dim3(AGG_BLOCK), 0, st, (const int32_t *)dv, rows, is_float, d_stats); break;
                default: hipLaunchKernelGGL(wstats_kernel<int64_t>, dim3(grid), dim3(AGG_BLOCK), 0, st, (const int64_t *)dv, rows, is_float, d_stats); break;
            }
            WTRY(hipGetLastError());
        }
        WStats hs;
        WTRY(hipMemcpyAsync(&hs, d_stats, sizeof(hs), hipMemcpyDeviceToHost, st));
        WTRY(hipStreamSynchronize(st));
        oc.min_i = hs.mn;
        oc.max_i = hs.mx;
        /* TEXT: the host writer records C-collation lex-key min/max
         * (format.h csf_text_lex_key); this stats kernel reduces raw
         * integer order, so device-written TEXT chunks stay conservatively
         * unprunable rather than carry a wrong-order range */
        if (types[c] == CSTRIPE_TEXT) oc.has_min_max = false;

        const uint64_t raw_bytes = (uint64_t)rows * width;
        bool emitted = false;
        if (width == 8 && rows >= 3 && hs.xsig != 0) {
            int hb = 63;
            while (hb > 0 && !((hs.xsig >> hb) & 1)) hb--;
            const uint32_t L = (uint32_t)(hb / 8 + 1);
            if (L <= 4) {
                const uint64_t csz = (11ull + L) + (uint64_t)(rows - 3) * (L + 3) + 9;
                if (csz < raw_bytes) {
                    if (d_out_cap < csz) {
                        if (d_out) WTRY(hipFree(d_out));
                        d_out_cap = (csz + 4095) & ~4095ull;
                        WTRY(hipMalloc(&d_out, d_out_cap));
                    }
                    hipLaunchKernelGGL(wemit_p_kernel,
                                       dim3((rows + AGG_BLOCK - 1) / AGG_BLOCK),
                                       dim3(AGG_BLOCK), 0, st,
                                       (const uint64_t *)dv, rows, L, d_out);
                    WTRY(hipGetLastError());
                    oc.data.resize(csz);
                    WTRY(hipMemcpyAsync(oc.data.data(), d_out, csz, hipMemcpyDeviceToHost, st));
                    WTRY(hipStreamSynchronize(st));
                    oc.mode = (uint8_t)(CSF_SEGMODE_P_BASE | L);
                    oc.canonical = true;
                    emitted = true;
                }
            }
        } else if (width == 8 && rows >= 3 && hs.xsig == 0) {
            /* constant chunk: emit on host from v0 (8 bytes over PCIe) */
            uint64_t v0;
            WTRY(hipMemcpyAsync(&v0, dv, 8, hipMemcpyDeviceToHost, st));
            WTRY(hipStreamSynchronize(st));
            oc.data.resize(64 + rows / 16);
            int csz = lz4e_canon_const((const uint8_t *)&v0, (int)rows,
                                       oc.data.data(), (int)oc.data.size());
            if (csz > 0 && (uint64_t)csz < raw_bytes) {
                oc.data.resize((size_t)csz);
                oc.mode = CSF_SEGMODE_CONST;
                oc.canonical = true;
                emitted = true;
            }
        }
        if (!emitted) {
            /* raw copy-back: the host writer path compresses it */
            oc.data.resize(raw_bytes);
            if (raw_bytes) {
                WTRY(hipMemcpyAsync(oc.data.data(), dv, raw_bytes, hipMemcpyDeviceToHost, st));
                WTRY(hipStreamSynchronize(st));
            }
            oc.canonical = false;
        }
    }
    #undef WTRY
    cleanup();
    return CSTRIPE_OK;
}

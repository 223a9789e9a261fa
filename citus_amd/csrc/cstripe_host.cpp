/*
 * cstripe_host.cpp — host side of the MI355X-native columnar scan path:
 * format producer (writer), flat-file stripe directory (reader/footer),
 * chunk-group min/max pruning, and the combine surface.
 *
 * Reference semantics restated (never copied) from:
 *   writer:  columnar_writer.c  ColumnarWriteRow :168-266, FlushStripe
 *            :391-516, SerializeBoolArray :523-545, SerializeSingleDatum
 *            :555-585, SerializeChunkData :592-654, UpdateChunkSkipNodeMinMax
 *            :663-718
 *   codec:   columnar_compression.c CompressBuffer :62-158 (lz4 :71-94,
 *            zstd :97-121), DecompressBuffer :165-270
 *   pruning: columnar_reader.c SelectedChunkMask :1132-1187 (range
 *            refutation per qual var; count a chunk once)
 *   combine: distributed/utils/aggregate_utils.c coord_combine_agg core
 *            :820-1021 (strict: skip NULL partials, first non-NULL
 *            initializes); COUNT NULL->0 COALESCE
 *            multi_logical_optimizer.c:1831-1885
 */
#include "internal.h"
#include "compress.h"
#include "lz4_enc.h"
#include "pglz.h"
#include "zstd_r.h"
#include "vartext.h"
#include "like.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <dirent.h>
#include <string>
#include <unistd.h>

#ifdef _OPENMP
#include <omp.h>
#endif

/* ============================ errors ============================ */

static thread_local char g_errbuf[512] = "";

void cs_set_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_errbuf, sizeof(g_errbuf), fmt, ap);
    va_end(ap);
}

extern "C" const char *cstripe_errmsg(void) { return g_errbuf; }
extern "C" uint32_t cstripe_abi_version(void) { return CSTRIPE_ABI_VERSION; }

extern "C" void cstripe_default_options(cstripe_options *o)
{
    /* defaults mirror columnar.c:30-44 (stripe 150000, chunk 10000, level 3;
     * default codec here is LZ4 — the GPU decode path's native codec) */
    o->stripe_row_limit = 150000;
    o->chunk_group_row_limit = 10000;
    o->compression = CSTRIPE_COMP_LZ4;
    o->compression_level = 3;
    o->lz4_seg_target_kb = 0;
    o->lz4_seg_target_bytes = 256;
    o->lz4_min_match = 4;              /* standard greedy LZ4 parse */
    o->canonical = 1;                  /* closed-form canonical parses on */
}

static uint32_t type_width(uint8_t t) { return csf_type_width(t); }

/* PG float ordering (backend/utils/adt/float.c float8_cmp_internal):
 * NaN sorts greater than every non-NaN and equal to itself. Used for
 * writer min/max skip nodes and for chunk refutation so float pruning
 * matches the reference's operator semantics (round-1 advisor finding). */
static inline int f64_cmp_pg(double a, double b)
{
    if (a > b) return 1;
    if (a < b) return -1;
    if (a == b) return 0;
    const bool na = (a != a), nb = (b != b);
    if (na && nb) return 0;
    return na ? 1 : -1;
}

/* ============================ writer ============================ */

namespace {

struct ChunkOut {
    std::vector<uint8_t> exists_packed;
    std::vector<uint8_t> value_comp;      /* compressed (or raw) value stream */
    std::vector<csf_seg> segs;
    csf_skipnode node;                    /* offsets filled at flush */
};

struct ColCur {
    std::vector<uint8_t> values;          /* packed present values, current chunk */
    std::vector<uint8_t> exists;          /* 1 byte per row, current chunk */
    bool has_min_max = false;
    int64_t min_i = 0, max_i = 0;         /* physical encoding (f64 via bit pattern) */
    std::vector<uint8_t> raw_pending;     /* finalized raw value streams, pending compress */
    /* VARTEXT: memcmp-smallest / -largest value of the current chunk; the
     * skip node stores their prefix keys (vartext.h) */
    std::string min_s, max_s;
};

struct PendingChunk {                     /* raw chunk awaiting compression at flush */
    uint32_t col;
    uint32_t chunk;
    std::vector<uint8_t> raw_values;
    std::vector<uint8_t> exists_packed;
    csf_skipnode node;                    /* min/max/row_count/n_present/decomp filled */
    /* device write path: stream already compressed on the GPU */
    bool has_ready = false;
    std::vector<uint8_t> ready_comp;
    uint8_t ready_mode = 0;
};

} /* namespace */

struct cstripe_writer {
    FILE *f = nullptr;
    std::string path;
    std::vector<csf_coldef> cols;
    cstripe_options opts{};
    uint64_t file_pos = 0;
    uint64_t total_rows = 0;

    /* current stripe */
    uint64_t stripe_first_row = 0;
    uint32_t stripe_rows = 0;             /* rows accumulated in current stripe */
    std::vector<ColCur> cur;              /* per column, current chunk state */
    std::vector<PendingChunk> pending;    /* finalized raw chunks of current stripe */
    std::vector<uint32_t> chunk_rows;     /* rows per finalized chunk */

    /* footer accumulation */
    std::vector<cs_stripe_info> stripes;

    bool vartext_bad = false;             /* a serialized VARTEXT chunk failed
                                           * its own header walk */
};

/* typed min/max update over a span of present values */
static void update_minmax(ColCur &c, uint8_t type, const uint8_t *vals, size_t n)
{
    if (n == 0) return;
    switch (type) {
        case CSTRIPE_I8: {
            const int8_t *v = (const int8_t *)vals;
            int8_t mn = v[0], mx = v[0];
            for (size_t i = 1; i < n; i++) { if (v[i] < mn) mn = v[i]; if (v[i] > mx) mx = v[i]; }
            if (!c.has_min_max) { c.min_i = mn; c.max_i = mx; c.has_min_max = true; }
            else { if (mn < (int8_t)c.min_i) c.min_i = mn; if (mx > (int8_t)c.max_i) c.max_i = mx; }
            break;
        }
        case CSTRIPE_I16: {
            const int16_t *v = (const int16_t *)vals;
            int16_t mn = v[0], mx = v[0];
            for (size_t i = 1; i < n; i++) { if (v[i] < mn) mn = v[i]; if (v[i] > mx) mx = v[i]; }
            if (!c.has_min_max) { c.min_i = mn; c.max_i = mx; c.has_min_max = true; }
            else { if (mn < (int16_t)c.min_i) c.min_i = mn; if (mx > (int16_t)c.max_i) c.max_i = mx; }
            break;
        }
        case CSTRIPE_I32: {
            const int32_t *v = (const int32_t *)vals;
            int32_t mn = v[0], mx = v[0];
            for (size_t i = 1; i < n; i++) { if (v[i] < mn) mn = v[i]; if (v[i] > mx) mx = v[i]; }
            if (!c.has_min_max) { c.min_i = mn; c.max_i = mx; c.has_min_max = true; }
            else { if (mn < (int32_t)c.min_i) c.min_i = mn; if (mx > (int32_t)c.max_i) c.max_i = mx; }
            break;
        }
        case CSTRIPE_I64: {
            const int64_t *v = (const int64_t *)vals;
            int64_t mn = v[0], mx = v[0];
            for (size_t i = 1; i < n; i++) { if (v[i] < mn) mn = v[i]; if (v[i] > mx) mx = v[i]; }
            if (!c.has_min_max) { c.min_i = mn; c.max_i = mx; c.has_min_max = true; }
            else { if (mn < c.min_i) c.min_i = mn; if (mx > c.max_i) c.max_i = mx; }
            break;
        }
        case CSTRIPE_F32: {
            const float *v = (const float *)vals;
            double mn = v[0], mx = v[0];
            for (size_t i = 1; i < n; i++) {
                if (f64_cmp_pg(v[i], mn) < 0) mn = v[i];
                if (f64_cmp_pg(v[i], mx) > 0) mx = v[i];
            }
            if (!c.has_min_max) { memcpy(&c.min_i, &mn, 8); memcpy(&c.max_i, &mx, 8); c.has_min_max = true; }
            else {
                double omn, omx; memcpy(&omn, &c.min_i, 8); memcpy(&omx, &c.max_i, 8);
                if (f64_cmp_pg(mn, omn) < 0) memcpy(&c.min_i, &mn, 8);
                if (f64_cmp_pg(mx, omx) > 0) memcpy(&c.max_i, &mx, 8);
            }
            break;
        }
        case CSTRIPE_F64: {
            const double *v = (const double *)vals;
            double mn = v[0], mx = v[0];
            for (size_t i = 1; i < n; i++) {
                if (f64_cmp_pg(v[i], mn) < 0) mn = v[i];
                if (f64_cmp_pg(v[i], mx) > 0) mx = v[i];
            }
            if (!c.has_min_max) { memcpy(&c.min_i, &mn, 8); memcpy(&c.max_i, &mx, 8); c.has_min_max = true; }
            else {
                double omn, omx; memcpy(&omn, &c.min_i, 8); memcpy(&omx, &c.max_i, 8);
                if (f64_cmp_pg(mn, omn) < 0) memcpy(&c.min_i, &mn, 8);
                if (f64_cmp_pg(mx, omx) > 0) memcpy(&c.max_i, &mx, 8);
            }
            break;
        }
        case CSTRIPE_TEXT: {
            /* min/max in the C-collation lex-key order (format.h
             * csf_text_lex_key) — used for EQ/NE refutation only */
            const uint32_t *v = (const uint32_t *)vals;
            int64_t mn = csf_text_lex_key(v[0]), mx = mn;
            for (size_t i = 1; i < n; i++) {
                const int64_t k = csf_text_lex_key(v[i]);
                if (k < mn) mn = k;
                if (k > mx) mx = k;
            }
            if (!c.has_min_max) { c.min_i = mn; c.max_i = mx; c.has_min_max = true; }
            else { if (mn < c.min_i) c.min_i = mn; if (mx > c.max_i) c.max_i = mx; }
            break;
        }
    }
}

/* SerializeBoolArray (columnar_writer.c:523-545): bit i of byte i/8, LSB first */
static std::vector<uint8_t> pack_bools(const std::vector<uint8_t> &b)
{
    size_t n = b.size();
    std::vector<uint8_t> out((n + 7) / 8, 0);
    for (size_t i = 0; i < n; i++)
        if (b[i]) out[i / 8] |= (uint8_t)(1u << (i % 8));
    return out;
}

extern "C" cstripe_writer *cstripe_write_begin(const char *path, const cstripe_coldef *cols,
                                               uint32_t n_cols, const cstripe_options *opts)
{
    if (!path || !cols || n_cols == 0 || n_cols > 64) { cs_set_err("write_begin: bad args"); return nullptr; }
    FILE *f = fopen(path, "wb");
    if (!f) { cs_set_err("write_begin: cannot open %s", path); return nullptr; }

    auto *w = new cstripe_writer();
    w->f = f;
    w->path = path;
    if (opts) w->opts = *opts; else cstripe_default_options(&w->opts);
    if (w->opts.lz4_seg_target_bytes == 0 && w->opts.lz4_seg_target_kb == 0)
        w->opts.lz4_seg_target_bytes = 256;
    /* segment decomp_len carries the stream-shape mode in bits 24-31, so a
     * single-segment chunk's raw stream must fit 24 bits (default 10000-row
     * chunks are 80 KB; 1M rows x 8 B = 8 MB still fits with margin) */
    if ((uint64_t)w->opts.chunk_group_row_limit * 8 >= (1u << 24) ||
        w->opts.chunk_group_row_limit == 0) {
        cs_set_err("chunk_group_row_limit %u out of range (1 .. 2097151)",
                   w->opts.chunk_group_row_limit);
        fclose(f);
        delete w;
        return nullptr;
    }
    for (uint32_t i = 0; i < n_cols; i++) {
        csf_coldef d{};
        memcpy(d.name, cols[i].name, sizeof(d.name));
        d.name[31] = 0;
        d.type = cols[i].type;
        d.scale = cols[i].scale;
        if (type_width(d.type) == 0) { cs_set_err("write_begin: bad column type %d", d.type); fclose(f); delete w; return nullptr; }
        w->cols.push_back(d);
    }
    w->cur.resize(n_cols);

    uint8_t hdr[CSF_HEADER_SIZE] = {0};
    memcpy(hdr, CSF_MAGIC, 8);
    uint32_t ver = CSF_VERSION;
    memcpy(hdr + 8, &ver, 4);
    fwrite(hdr, 1, CSF_HEADER_SIZE, f);
    w->file_pos = CSF_HEADER_SIZE;
    return w;
}

/* finalize the current chunk of every column into w->pending (raw; compression
 * deferred to flush so it can run in parallel across chunks) */
static void finalize_chunk(cstripe_writer *w, uint32_t rows_in_chunk)
{
    uint32_t chunk_index = (uint32_t)w->chunk_rows.size();
    for (uint32_t c = 0; c < w->cols.size(); c++) {
        ColCur &cc = w->cur[c];
        PendingChunk pc;
        pc.col = c;
        pc.chunk = chunk_index;
        pc.raw_values = std::move(cc.values);
        pc.exists_packed = pack_bools(cc.exists);
        memset(&pc.node, 0, sizeof(pc.node));
        pc.node.min_i = cc.min_i;
        pc.node.max_i = cc.max_i;
        pc.node.has_min_max = cc.has_min_max ? 1 : 0;
        pc.node.row_count = rows_in_chunk;
        uint32_t width = type_width(w->cols[c].type);
        pc.node.n_present = (uint32_t)(pc.raw_values.size() / width);
        if (w->cols[c].type == CSTRIPE_VARTEXT) {
            uint32_t np = 0;
            for (uint8_t e : cc.exists) np += e;
            pc.node.n_present = np;
            if (cc.has_min_max) {
                pc.node.min_i = csvt_prefix_key((const uint8_t *)cc.min_s.data(), (uint32_t)cc.min_s.size());
                pc.node.max_i = csvt_prefix_key((const uint8_t *)cc.max_s.data(), (uint32_t)cc.max_s.size());
            }
            /* self-check: the stream just serialized must walk back to
             * exactly n_present datums (the reader's header walk) */
            if (csvt_validate(pc.raw_values.data(), pc.raw_values.size(), np) != 0)
                w->vartext_bad = true;
            cc.min_s.clear();
            cc.max_s.clear();
        }
        pc.node.decompressed_size = pc.raw_values.size();
        w->pending.push_back(std::move(pc));
        cc.values.clear();
        cc.exists.clear();
        cc.has_min_max = false;
        cc.min_i = cc.max_i = 0;
    }
    w->chunk_rows.push_back(rows_in_chunk);
}

/* compress one pending chunk's value stream into out (segments); mirrors
 * SerializeChunkData/CompressBuffer: lz4/zstd per segment, raw when the codec
 * is NONE or fails. Returns false only on a hard format-capacity error
 * (> CSF segment cap), never on incompressible data. */
static bool compress_chunk(const cstripe_writer *w, const PendingChunk &pc, ChunkOut &out)
{
    out.node = pc.node;
    out.exists_packed = pc.exists_packed;
    if (pc.has_ready) {                   /* GPU-compressed canonical stream */
        out.value_comp = pc.ready_comp;
        csf_seg s{0, (uint32_t)pc.ready_comp.size(), 0,
                  (uint32_t)pc.node.decompressed_size |
                  ((uint32_t)pc.ready_mode << 24)};
        out.segs.push_back(s);
        out.node.comp_type = CSTRIPE_COMP_LZ4;
        out.node.comp_level = 0;
        out.node.n_segs = 1;
        out.node.value_len = pc.ready_comp.size();
        return true;
    }
    const std::vector<uint8_t> &raw = pc.raw_values;
    uint8_t codec = w->opts.compression;
    size_t target = w->opts.lz4_seg_target_bytes ? w->opts.lz4_seg_target_bytes
                                                 : (size_t)w->opts.lz4_seg_target_kb * 1024;
    uint32_t width = type_width(w->cols[pc.col].type);
    if (w->cols[pc.col].type == CSTRIPE_VARTEXT)
        width = 1;      /* a byte stream: no canonical parse applies, matches
                         * at any distance (generic segment paths only) */
    if (width == 1 && raw.size() >= (1u << 24)) {
        /* a segment's decomp_len keeps 24 bits (format.h) */
        cs_set_err("VARTEXT chunk stream of %zu bytes (max 16 MiB - 1): lower "
                   "chunk_group_row_limit", raw.size());
        return false;
    }

    if (codec == CSTRIPE_COMP_PGLZ && !raw.empty()) {
        /* reference PG_LZ layout: ColumnarCompressHeader (varlena len +
         * rawsize) then the pglz stream, one whole-chunk buffer
         * (columnar_compression.c:122-151) */
        out.value_comp.resize(raw.size() + CSPGLZ_HDRSZ);
        int32_t csz = cspglz_compress(raw.data(), (int32_t)raw.size(),
                                      out.value_comp.data() + CSPGLZ_HDRSZ,
                                      (int32_t)raw.size());
        if (csz > 0) {
            out.value_comp.resize((size_t)csz + CSPGLZ_HDRSZ);
            cspglz_set_header(out.value_comp.data(),
                              (uint32_t)out.value_comp.size(),
                              (int32_t)raw.size());
            csf_seg s{0, (uint32_t)out.value_comp.size(), 0, (uint32_t)raw.size()};
            out.segs.push_back(s);
            out.node.comp_type = CSTRIPE_COMP_PGLZ;
            out.node.comp_level = 0;
            out.node.n_segs = 1;
            out.node.value_len = out.value_comp.size();
            return true;
        }
        out.value_comp.clear();
        codec = CSTRIPE_COMP_NONE;      /* did not shrink -> raw */
    }
    if (raw.empty() || codec == CSTRIPE_COMP_NONE) {
        out.value_comp = raw;
        csf_seg s{0, (uint32_t)raw.size(), 0, (uint32_t)raw.size()};
        out.segs.push_back(s);
        out.node.comp_type = CSTRIPE_COMP_NONE;
        out.node.comp_level = 0;
        out.node.n_segs = 1;
        out.node.value_len = raw.size();
        return true;
    }

    /* ---- canonical parses (closed-form GPU access; see format.h) ----
     * The emitted stream is a standard LZ4 block / zstd frame either way;
     * canonical just picks a parse whose value positions are computable,
     * killing the GPU's per-sequence/FSE parse chain (round-1's instruction
     * wall). */
    if ((codec == CSTRIPE_COMP_LZ4 || codec == CSTRIPE_COMP_ZSTD) &&
        w->opts.canonical && width == 8 &&
        raw.size() >= 24 && raw.size() < (1u << 24) &&
        (codec == CSTRIPE_COMP_LZ4 || raw.size() < (127u << 10))) {
        const size_t nv = raw.size() / 8;
        uint64_t v0, x = 0;
        memcpy(&v0, raw.data(), 8);
        const uint8_t *rp = raw.data();
        for (size_t i = 1; i < nv; i++) {
            uint64_t vi;
            memcpy(&vi, rp + i * 8, 8);
            x |= vi ^ v0;
        }
        static const zr_ctables zct_c = [] {
            zr_ctables t;
            zr_build_ctables(&t);
            return t;
        }();
        int mode = -1, csz = 0;
        size_t cap = raw.size() + raw.size() / 8 + 64;
        out.value_comp.resize(cap);
        if (x == 0) {
            if (codec == CSTRIPE_COMP_LZ4) {
                csz = lz4e_canon_const(rp, (int)nv, out.value_comp.data(), (int)cap);
                if (csz > 0) mode = CSF_SEGMODE_CONST;
            } else {
                csz = zr_canon_const(rp, (int)nv, out.value_comp.data(), (int)cap, &zct_c);
                if (csz > 0) mode = CSF_SEGMODE_ZR_CONST;
            }
        } else {
            int L = (63 - __builtin_clzll(x)) / 8 + 1;
            if (L <= 4) {
                if (codec == CSTRIPE_COMP_LZ4) {
                    csz = lz4e_canon_p(rp, (int)nv, L, out.value_comp.data(), (int)cap);
                    if (csz > 0) mode = (int)(CSF_SEGMODE_P_BASE | (uint32_t)L);
                } else {
                    csz = zr_canon_p(rp, (int)nv, L, out.value_comp.data(), (int)cap, &zct_c);
                    if (csz > 0) mode = (int)(CSF_SEGMODE_ZRP_BASE | (uint32_t)L);
                }
            }
            /* L > 4: high bytes vary — no canonical parse; the greedy path
             * below runs, and its incompressible->NONE fallback (reference
             * CompressBuffer semantics) already yields closed-form access */
        }
        if (mode >= 0 && (size_t)csz >= raw.size())
            mode = -1;   /* did not shrink -> raw NONE below (reference rule) */
        if (mode >= 0) {
            out.value_comp.resize((size_t)csz);
            csf_seg s{0, (uint32_t)csz, 0,
                      (uint32_t)raw.size() | ((uint32_t)mode << 24)};
            out.segs.push_back(s);
            out.node.comp_type = codec;
            out.node.comp_level = 0;
            out.node.n_segs = 1;
            out.node.value_len = (uint64_t)csz;
            return true;
        }
    }

    /* width-4 canonical zstd: slots that differ in at most ONE byte (the
     * char(1) short-varlena case: [0x05 ch 00 00] varies only in byte 1) —
     * expressible in zstd (min match 3) but not LZ4 (min match 4); the GPU
     * reads one byte per row closed-form (csf_canon_zr4b_pos) */
    if (codec == CSTRIPE_COMP_ZSTD && w->opts.canonical && width == 4 &&
        raw.size() >= 12 && raw.size() < (127u << 10)) {
        const size_t nv = raw.size() / 4;
        uint32_t v0, x = 0;
        memcpy(&v0, raw.data(), 4);
        const uint8_t *rp = raw.data();
        for (size_t i = 1; i < nv; i++) {
            uint32_t vi;
            memcpy(&vi, rp + i * 4, 4);
            x |= vi ^ v0;
        }
        static const zr_ctables zct4 = [] {
            zr_ctables t;
            zr_build_ctables(&t);
            return t;
        }();
        int mode = -1, csz = 0, k = -1;
        if (x == 0) {
            k = 4;                           /* const form */
        } else {
            for (int b = 0; b < 4; b++)
                if ((x & ~(0xFFu << (8 * b))) == 0) { k = b; break; }
        }
        if (k >= 0) {
            size_t cap = raw.size() + 64;
            out.value_comp.resize(cap);
            if (k == 4) {
                csz = zr_canon_const4(rp, (int)nv, out.value_comp.data(), (int)cap, &zct4);
                if (csz > 0) mode = CSF_SEGMODE_ZR4_CONST;
            } else {
                csz = zr_canon_b4(rp, (int)nv, k, out.value_comp.data(), (int)cap, &zct4);
                if (csz > 0) mode = (int)(CSF_SEGMODE_ZR4B_BASE | (uint32_t)k);
            }
        }
        if (mode >= 0 && (size_t)csz >= raw.size())
            mode = -1;
        if (mode >= 0) {
            out.value_comp.resize((size_t)csz);
            csf_seg s{0, (uint32_t)csz, 0,
                      (uint32_t)raw.size() | ((uint32_t)mode << 24)};
            out.segs.push_back(s);
            out.node.comp_type = codec;
            out.node.comp_level = 0;
            out.node.n_segs = 1;
            out.node.value_len = (uint64_t)csz;
            return true;
        }
        out.value_comp.clear();
    }

    /* segment boundaries 16 B-aligned (pure byte split of the raw stream;
     * lets the GPU flush decoded segments with aligned 16 B stores) */
    (void)width;
    size_t n = raw.size();
    size_t per = (target / 16) * 16;    /* exact target (16B-aligned splits) —
                                         * uniform segments are what the fused
                                         * GPU kernel's tile math assumes */
    if (codec == CSTRIPE_COMP_ZSTD && per < 256)
        per = 256;                      /* ~13 B frame overhead (5%) is worth
                                         * the GPU decoder occupancy: LDS
                                         * bytes/frame bound waves/CU, and
                                         * 256 B frames double them vs 512 */
    if (per == 0) per = n;
    if (w->cols[pc.col].type == CSTRIPE_VARTEXT) {
        /* text is decoded once per stage into a temporary buffer, never by
         * the fused 256 B lane-region kernels, so it takes the largest
         * segment the lane-parallel decoders still handle: a 4x longer match
         * window for strings that repeat across rows */
        if (per < 1024) per = 1024;
        if ((n + per - 1) / per > 4096)
            per = (((n + 4095) / 4096) + 15) / 16 * 16;   /* long strings: stay
                                                           * under the 4096-
                                                           * segment cap */
    }
    /* caps: segment decomp_len carries the mode byte in bits 24-31 (8 MB is
     * comfortably under 2^24), and a restricted-zstd RAW-block fallback is
     * bounded by the 21-bit block size (1 MB) */
    if (per > (1u << 23)) per = 1u << 23;
    if (codec == CSTRIPE_COMP_ZSTD && per > (96u << 10))
        per = 96u << 10;               /* zstd block content cap is 128 KB */

    out.value_comp.clear();
    out.segs.clear();
    size_t off = 0;
    bool ok = true;
    lz4e_state enc;                   /* one init per chunk, reused across
                                       * segments (see lz4_enc.h) */
    if (codec == CSTRIPE_COMP_LZ4) lz4e_init(&enc);
    while (off < n) {
        size_t len = std::min(per, n - off);
        /* absorb a tiny (<16 B) tail only in large-segment mode: the GPU
         * fused/lane kernels assume non-final segments are EXACTLY `per`
         * decompressed bytes and the final one is <= per, so for the
         * 256 B lane-parallel default a 257-271 B absorbed final segment
         * would be read from the wrong lane region (round-1 advisor
         * finding); a standalone <16 B final segment decodes fine */
        if (per > 256 && n - off - len < 16) len = n - off;
        csf_seg s{};
        s.decomp_off = (uint32_t)off;
        s.decomp_len = (uint32_t)len;
        s.comp_off = (uint32_t)out.value_comp.size();
        if (codec == CSTRIPE_COMP_LZ4) {
            int bound = LZ4_compressBound((int)len);
            size_t base = out.value_comp.size();
            out.value_comp.resize(base + (size_t)bound);
            /* width-granular matches for 4-byte slot streams (TEXT/I32/F32):
             * the GPU lane decoder's aligned-word path then covers every copy */
            const int malign = (width == 4) ? 4 : 1;
            int csz = lz4e_compress_mm_a(&enc, raw.data() + off,
                                         (int)len, out.value_comp.data() + base, bound,
                                         w->opts.lz4_min_match >= 4 ? w->opts.lz4_min_match : 4,
                                         malign);
            if (csz <= 0)             /* capacity fallback: system liblz4 */
                csz = LZ4_compress_default((const char *)raw.data() + off,
                                           (char *)out.value_comp.data() + base,
                                           (int)len, bound);
            if (csz <= 0) { ok = false; break; }
            out.value_comp.resize(base + (size_t)csz);
            s.comp_len = (uint32_t)csz;
        } else if (codec == CSTRIPE_COMP_ZSTD) {
            /* restricted zstd frames (zstd_r.h): standard RFC 8878 frames
             * the GPU lane decoder handles (raw literals + predefined-FSE
             * sequences); libzstd-decodable, pinned in tests. Falls back to
             * a raw-block frame when the parse does not shrink a segment. */
            /* magic static: thread-safe one-time build (C++11) */
            static const zr_ctables zct = [] {
                zr_ctables t;
                zr_build_ctables(&t);
                return t;
            }();
            size_t bound = (size_t)len + len / 2 + 64;
            size_t base = out.value_comp.size();
            out.value_comp.resize(base + bound);
            int csz = zr_compress(raw.data() + off, (int)len,
                                  out.value_comp.data() + base, (int)bound, &zct);
            if (csz <= 0) {
                /* raw-block frame: magic+fhd+fcs+bh then the bytes */
                uint8_t *d = out.value_comp.data() + base;
                int op2 = 0;
                d[op2++] = 0x28; d[op2++] = 0xB5; d[op2++] = 0x2F; d[op2++] = 0xFD;
                if (len <= 255) { d[op2++] = 0x20; d[op2++] = (uint8_t)len; }
                else if (len <= 65535 + 256) {
                    d[op2++] = 0x60;
                    uint32_t f2 = (uint32_t)len - 256;
                    d[op2++] = (uint8_t)f2; d[op2++] = (uint8_t)(f2 >> 8);
                } else {
                    d[op2++] = 0xA0;
                    uint32_t f2 = (uint32_t)len;
                    d[op2++] = (uint8_t)f2; d[op2++] = (uint8_t)(f2 >> 8);
                    d[op2++] = (uint8_t)(f2 >> 16); d[op2++] = (uint8_t)(f2 >> 24);
                }
                uint32_t bh = 1u | (0u << 1) | ((uint32_t)len << 3);
                d[op2++] = (uint8_t)bh; d[op2++] = (uint8_t)(bh >> 8); d[op2++] = (uint8_t)(bh >> 16);
                memcpy(d + op2, raw.data() + off, len);
                csz = op2 + (int)len;
            }
            out.value_comp.resize(base + (size_t)csz);
            s.comp_len = (uint32_t)csz;
            s.decomp_len |= CSF_SEGMODE_ZR << 24;
        } else {
            ok = false; break;
        }
        out.segs.push_back(s);
        off += len;
    }

    /* incompressible -> keep raw, like the reference (CompressBuffer returns
     * false when compression does not shrink, columnar_compression.c:88-94;
     * raw NONE chunks also get closed-form GPU access for free) */
    if (ok && out.value_comp.size() >= raw.size())
        ok = false;
    if (!ok) {  /* CompressBuffer returned false -> keep uncompressed */
        out.value_comp = raw;
        out.segs.clear();
        csf_seg s{0, (uint32_t)raw.size(), 0, (uint32_t)raw.size()};
        out.segs.push_back(s);
        out.node.comp_type = CSTRIPE_COMP_NONE;
        out.node.comp_level = 0;
    } else {
        out.node.comp_type = codec;
        out.node.comp_level = w->opts.compression_level;
    }
    /* reader cap is 4096 segments and n_segs is uint16 — refuse to emit a
     * chunk the reader would reject (or, after wraparound, misparse) instead
     * of silently truncating (round-1 advisor finding) */
    if (out.segs.size() > 4096) {
        cs_set_err("chunk needs %zu segments (> 4096 cap): raise "
                   "lz4_seg_target_bytes or lower chunk_group_row_limit",
                   out.segs.size());
        return false;
    }
    out.node.n_segs = (uint16_t)out.segs.size();
    out.node.value_len = out.value_comp.size();
    return true;
}

/* FlushStripe (columnar_writer.c:391-516): compress pending chunks, lay out
 * per column all exists streams then all value streams, offsets relative to
 * stripe data start; append stripe metadata for the footer */
static int flush_stripe(cstripe_writer *w)
{
    if (w->stripe_rows == 0) return CSTRIPE_OK;
    /* finalize a partial last chunk (FlushStripe :419-422) */
    uint32_t done_rows = 0;
    for (uint32_t r : w->chunk_rows) done_rows += r;
    if (done_rows < w->stripe_rows)
        finalize_chunk(w, w->stripe_rows - done_rows);

    if (w->vartext_bad) {
        cs_set_err("flush: a serialized VARTEXT chunk failed its own header walk");
        return CSTRIPE_ERR_FORMAT;
    }

    uint32_t n_cols = (uint32_t)w->cols.size();
    uint32_t n_chunks = (uint32_t)w->chunk_rows.size();

    /* compress all pending chunks (parallel; independent per column-chunk) */
    std::vector<ChunkOut> outs(w->pending.size());
    bool comp_ok = true;
    #pragma omp parallel for schedule(dynamic)
    for (long i = 0; i < (long)w->pending.size(); i++)
        if (!compress_chunk(w, w->pending[i], outs[i]))
            comp_ok = false;
    if (!comp_ok) {
        /* compress_chunk set the detailed message on its OMP worker thread's
         * buffer; restate on the caller's thread where errmsg() reads */
        cs_set_err("chunk exceeds the 4096-segment cap: raise "
                   "lz4_seg_target_bytes or lower chunk_group_row_limit");
        return CSTRIPE_ERR_FORMAT;
    }

    /* outs indexed by pending order: chunk-major (all columns of chunk 0, then
     * chunk 1, ...). Reorder access as [col][chunk]. */
    auto out_at = [&](uint32_t col, uint32_t chunk) -> ChunkOut & {
        return outs[(size_t)chunk * n_cols + col];
    };

    /* compute offsets: per column, exists streams then value streams
     * (FlushStripe :425-458) */
    uint64_t stripe_size = 0;
    for (uint32_t c = 0; c < n_cols; c++) {
        for (uint32_t k = 0; k < n_chunks; k++) {
            ChunkOut &o = out_at(c, k);
            o.node.exists_off = stripe_size;
            o.node.exists_len = o.exists_packed.size();
            stripe_size += o.exists_packed.size();
        }
        for (uint32_t k = 0; k < n_chunks; k++) {
            ChunkOut &o = out_at(c, k);
            o.node.value_off = stripe_size;
            stripe_size += o.node.value_len;
        }
    }

    uint64_t stripe_file_off = w->file_pos;

    /* write data: per column all exists, then all values (FlushStripe :477-502) */
    for (uint32_t c = 0; c < n_cols; c++) {
        for (uint32_t k = 0; k < n_chunks; k++) {
            ChunkOut &o = out_at(c, k);
            if (!o.exists_packed.empty() &&
                fwrite(o.exists_packed.data(), 1, o.exists_packed.size(), w->f) != o.exists_packed.size())
                { cs_set_err("flush: short write"); return CSTRIPE_ERR_IO; }
        }
        for (uint32_t k = 0; k < n_chunks; k++) {
            ChunkOut &o = out_at(c, k);
            if (!o.value_comp.empty() &&
                fwrite(o.value_comp.data(), 1, o.value_comp.size(), w->f) != o.value_comp.size())
                { cs_set_err("flush: short write"); return CSTRIPE_ERR_IO; }
        }
    }
    w->file_pos += stripe_size;

    /* record stripe for the footer */
    cs_stripe_info si;
    si.meta.file_offset = stripe_file_off;
    si.meta.data_size = stripe_size;
    si.meta.first_row_number = w->stripe_first_row;
    si.meta.row_count = w->stripe_rows;
    si.meta.chunk_count = n_chunks;
    si.meta.reserved = 0;
    si.group_rows = w->chunk_rows;
    si.nodes.resize(n_cols);
    for (uint32_t c = 0; c < n_cols; c++) {
        si.nodes[c].resize(n_chunks);
        for (uint32_t k = 0; k < n_chunks; k++) {
            si.nodes[c][k].n = out_at(c, k).node;
            si.nodes[c][k].segs = out_at(c, k).segs;
        }
    }
    w->stripes.push_back(std::move(si));

    /* reset stripe state */
    w->pending.clear();
    w->chunk_rows.clear();
    w->stripe_first_row += w->stripe_rows;
    w->stripe_rows = 0;
    return CSTRIPE_OK;
}

/* device-side append: full chunks compress on the GPU (csgpu_compress_chunk,
 * cstripe_gpu.hip); partial spans round-trip through the host accumulation
 * path to keep chunk/stripe boundary semantics identical */
extern "C" int cstripe_write_rows_device(cstripe_writer *w, uint64_t n_rows,
                                         const void *const *dev_values)
{
    if (!w || !dev_values) { cs_set_err("write_rows_device: bad args"); return CSTRIPE_ERR_ARG; }
    const uint32_t n_cols = (uint32_t)w->cols.size();
    const uint32_t chunk_limit = w->opts.chunk_group_row_limit;
    const uint64_t stripe_limit = w->opts.stripe_row_limit;
    std::vector<uint8_t> types(n_cols);
    for (uint32_t c = 0; c < n_cols; c++) types[c] = w->cols[c].type;
    for (uint32_t c = 0; c < n_cols; c++)
        if (types[c] == CSTRIPE_VARTEXT) {
            cs_set_err("write_rows_device: column %u is VARTEXT — variable-length "
                       "values go through cstripe_write_rows", c);
            return CSTRIPE_ERR_ARG;
        }

    uint64_t done = 0;
    while (done < n_rows) {
        const uint32_t in_chunk = (uint32_t)(w->stripe_rows % chunk_limit);
        const uint64_t to_chunk = chunk_limit - in_chunk;
        const uint64_t to_stripe = stripe_limit - w->stripe_rows;
        const uint64_t span = std::min({n_rows - done, to_chunk, to_stripe});

        const bool full_chunk = in_chunk == 0 && span == chunk_limit &&
                                w->opts.compression == CSTRIPE_COMP_LZ4 &&
                                w->opts.canonical;
        if (full_chunk) {
            std::vector<const void *> vp(n_cols);
            for (uint32_t c = 0; c < n_cols; c++) vp[c] = dev_values[c];
            std::vector<cs_dev_chunk_col> cc;
            int rc = csgpu_compress_chunk(vp.data(), types.data(), n_cols,
                                          (uint32_t)span, done, cc);
            if (rc != CSTRIPE_OK) return rc;
            const uint32_t chunk_index = (uint32_t)w->chunk_rows.size();
            std::vector<uint8_t> ones((span + 7) / 8, 0xFF);
            if (span % 8) ones.back() = (uint8_t)(0xFF >> (8 - span % 8));
            for (uint32_t c = 0; c < n_cols; c++) {
                PendingChunk pc;
                pc.col = c;
                pc.chunk = chunk_index;
                memset(&pc.node, 0, sizeof(pc.node));
                pc.node.min_i = cc[c].min_i;
                pc.node.max_i = cc[c].max_i;
                pc.node.has_min_max = cc[c].has_min_max ? 1 : 0;
                pc.node.row_count = span;
                pc.node.n_present = (uint32_t)span;
                pc.node.decompressed_size = span * type_width(types[c]);
                pc.exists_packed = ones;
                if (cc[c].canonical) {
                    pc.has_ready = true;
                    pc.ready_comp = std::move(cc[c].data);
                    pc.ready_mode = cc[c].mode;
                } else {
                    pc.raw_values = std::move(cc[c].data);
                }
                w->pending.push_back(std::move(pc));
            }
            w->chunk_rows.push_back((uint32_t)span);
            w->stripe_rows += (uint32_t)span;
            w->total_rows += span;
        } else {
            /* partial span / non-canonical codec: host accumulation path */
            std::vector<std::vector<uint8_t>> host(n_cols);
            std::vector<const void *> hp(n_cols);
            for (uint32_t c = 0; c < n_cols; c++) {
                const uint32_t width = type_width(types[c]);
                host[c].resize(span * width);
                if (hipMemcpy(host[c].data(),
                              (const uint8_t *)dev_values[c] + done * width,
                              span * width, hipMemcpyDeviceToHost) != hipSuccess) {
                    cs_set_err("write_rows_device: D2H copy failed");
                    return CSTRIPE_ERR;
                }
                hp[c] = host[c].data();
            }
            int rc = cstripe_write_rows(w, span, hp.data(), nullptr);
            if (rc != CSTRIPE_OK) return rc;
            done += span;
            continue;
        }
        done += span;
        if (w->stripe_rows >= stripe_limit) {
            int rc = flush_stripe(w);
            if (rc != CSTRIPE_OK) return rc;
        }
    }
    return CSTRIPE_OK;
}

extern "C" int cstripe_write_rows(cstripe_writer *w, uint64_t n_rows,
                                  const void *const *values, const uint8_t *const *nulls)
{
    if (!w || !values) { cs_set_err("write_rows: bad args"); return CSTRIPE_ERR_ARG; }
    uint32_t n_cols = (uint32_t)w->cols.size();
    const uint32_t chunk_limit = w->opts.chunk_group_row_limit;
    const uint64_t stripe_limit = w->opts.stripe_row_limit;

    /* VARTEXT values are checked for the whole batch before anything is
     * appended: payload <= CSTRIPE_VARTEXT_MAX_LEN, no NUL (PG text) */
    for (uint32_t c = 0; c < n_cols; c++) {
        if (w->cols[c].type != CSTRIPE_VARTEXT) continue;
        const cstripe_vartext_in *vt = (const cstripe_vartext_in *)values[c];
        if (!vt || !vt->offsets || (!vt->bytes && vt->offsets[n_rows] != vt->offsets[0])) {
            cs_set_err("write_rows: column %u is VARTEXT and needs a cstripe_vartext_in", c);
            return CSTRIPE_ERR_ARG;
        }
        const uint8_t *nl = (nulls && nulls[c]) ? nulls[c] : nullptr;
        for (uint64_t i = 0; i < n_rows; i++) {
            if (vt->offsets[i + 1] < vt->offsets[i]) {
                cs_set_err("write_rows: column %u row %llu: offsets decrease", c, (unsigned long long)i);
                return CSTRIPE_ERR_ARG;
            }
            if (nl && nl[i]) continue;
            const uint64_t len = vt->offsets[i + 1] - vt->offsets[i];
            if (len > CSTRIPE_VARTEXT_MAX_LEN) {
                cs_set_err("write_rows: column %u row %llu: text value of %llu bytes "
                           "(max %u)", c, (unsigned long long)i,
                           (unsigned long long)len, CSTRIPE_VARTEXT_MAX_LEN);
                return CSTRIPE_ERR_ARG;
            }
            if (len && memchr(vt->bytes + vt->offsets[i], 0, len)) {
                cs_set_err("write_rows: column %u row %llu: text value holds a NUL byte",
                           c, (unsigned long long)i);
                return CSTRIPE_ERR_ARG;
            }
        }
    }

    uint64_t done = 0;
    while (done < n_rows) {
        uint32_t in_chunk = w->stripe_rows % chunk_limit;
        uint64_t to_chunk = chunk_limit - in_chunk;
        uint64_t to_stripe = stripe_limit - w->stripe_rows;
        uint64_t span = std::min({n_rows - done, to_chunk, to_stripe});

        for (uint32_t c = 0; c < n_cols; c++) {
            ColCur &cc = w->cur[c];
            uint32_t width = type_width(w->cols[c].type);
            const uint8_t *src = (const uint8_t *)values[c] + done * width;
            const uint8_t *nl = (nulls && nulls[c]) ? nulls[c] + done : nullptr;
            if (w->cols[c].type == CSTRIPE_VARTEXT) {
                /* SerializeSingleDatum for a varlena, typalign 'i'
                 * (columnar_writer.c:555-585): short 1-byte header when the
                 * whole datum fits 127 bytes, else the 4-byte header; zero
                 * padding to the next 4-byte boundary */
                const cstripe_vartext_in *vt = (const cstripe_vartext_in *)values[c];
                size_t base = cc.exists.size();
                cc.exists.resize(base + span);
                for (uint64_t i = 0; i < span; i++) {
                    if (nl && nl[i]) { cc.exists[base + i] = 0; continue; }
                    cc.exists[base + i] = 1;
                    const uint8_t *pv = vt->bytes + vt->offsets[done + i];
                    const uint32_t len = (uint32_t)(vt->offsets[done + i + 1] - vt->offsets[done + i]);
                    if (len + 1 <= 127) {
                        cc.values.push_back((uint8_t)(((len + 1) << 1) | 1u));
                    } else {
                        const uint32_t h = (len + 4) << 2;
                        for (int b = 0; b < 4; b++) cc.values.push_back((uint8_t)(h >> (8 * b)));
                    }
                    if (len) cc.values.insert(cc.values.end(), pv, pv + len);
                    while (cc.values.size() & 3) cc.values.push_back(0);
                    /* memcmp order, shorter first on a prefix tie */
                    auto less = [](const uint8_t *a, uint32_t al, const std::string &b) {
                        const int r = memcmp(a, b.data(), std::min<size_t>(al, b.size()));
                        return r < 0 || (r == 0 && al < b.size());
                    };
                    auto greater = [](const uint8_t *a, uint32_t al, const std::string &b) {
                        const int r = memcmp(a, b.data(), std::min<size_t>(al, b.size()));
                        return r > 0 || (r == 0 && al > b.size());
                    };
                    if (!cc.has_min_max) {
                        cc.min_s.assign((const char *)pv, len);
                        cc.max_s = cc.min_s;
                        cc.has_min_max = true;
                    } else {
                        if (less(pv, len, cc.min_s)) cc.min_s.assign((const char *)pv, len);
                        if (greater(pv, len, cc.max_s)) cc.max_s.assign((const char *)pv, len);
                    }
                }
                continue;
            }
            if (w->cols[c].type == CSTRIPE_TEXT) {
                /* slots must be well-formed short varlena (hdr odd, total
                 * length 2..4 incl. header: payload <= 3 bytes) */
                for (uint64_t i = 0; i < span; i++) {
                    if (nl && nl[i]) continue;
                    const uint8_t hdr = src[i * 4];
                    const uint32_t tot = hdr >> 1;
                    if (!(hdr & 1) || tot < 2 || tot > 4) {
                        cs_set_err("text slot row %llu: not a short varlena "
                                   "with payload <= 3 bytes (hdr 0x%02x)",
                                   (unsigned long long)(done + i), hdr);
                        return CSTRIPE_ERR_ARG;
                    }
                }
            }
            size_t base = cc.exists.size();
            cc.exists.resize(base + span);
            if (!nl) {
                memset(cc.exists.data() + base, 1, span);
                size_t vbase = cc.values.size();
                cc.values.resize(vbase + span * width);
                memcpy(cc.values.data() + vbase, src, span * width);
                update_minmax(cc, w->cols[c].type, src, span);
            } else {
                for (uint64_t i = 0; i < span; i++) {
                    if (nl[i]) { cc.exists[base + i] = 0; continue; }
                    cc.exists[base + i] = 1;
                    size_t vbase = cc.values.size();
                    cc.values.resize(vbase + width);
                    memcpy(cc.values.data() + vbase, src + i * width, width);
                    update_minmax(cc, w->cols[c].type, src + i * width, 1);
                }
            }
        }

        w->stripe_rows += (uint32_t)span;
        w->total_rows += span;
        done += span;

        if (w->stripe_rows % chunk_limit == 0)
            finalize_chunk(w, chunk_limit);
        if (w->stripe_rows >= stripe_limit) {
            int rc = flush_stripe(w);
            if (rc != CSTRIPE_OK) return rc;
        }
    }
    return CSTRIPE_OK;
}

extern "C" int cstripe_vartext_validate(const uint8_t *stream, uint64_t len, uint32_t n_values)
{
    if (!stream && len) { cs_set_err("vartext_validate: null stream"); return CSTRIPE_ERR_ARG; }
    const int rc = csvt_validate(stream, len, n_values);
    if (rc == 0) return CSTRIPE_OK;
    static const char *const why[] = {"", "header form never written (compressed/external varlena)",
        "datum shorter than its header", "datum overruns the stream",
        "payload longer than CSTRIPE_VARTEXT_MAX_LEN", "fewer datums than n_values",
        "more datums than n_values"};
    cs_set_err("vartext stream (%llu bytes, %u values): %s",
               (unsigned long long)len, n_values, why[rc]);
    return CSTRIPE_ERR_FORMAT;
}

static void footer_append(std::vector<uint8_t> &buf, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    buf.insert(buf.end(), b, b + n);
}

extern "C" int cstripe_write_end(cstripe_writer *w)
{
    if (!w) return CSTRIPE_ERR_ARG;
    int rc = flush_stripe(w);
    if (rc != CSTRIPE_OK) { cstripe_write_abort(w); return rc; }

    std::vector<uint8_t> fb;
    csf_footer_head head{};
    head.version = CSF_VERSION;
    head.column_count = (uint32_t)w->cols.size();
    head.stripe_count = (uint32_t)w->stripes.size();
    head.chunk_row_limit = w->opts.chunk_group_row_limit;
    head.stripe_row_limit = w->opts.stripe_row_limit;
    head.total_rows = w->total_rows;
    head.compression = w->opts.compression;
    head.compression_level = w->opts.compression_level;
    head.lz4_seg_target_kb = w->opts.lz4_seg_target_kb;
    footer_append(fb, &head, sizeof(head));
    for (auto &c : w->cols) footer_append(fb, &c, sizeof(c));
    for (auto &s : w->stripes) {
        footer_append(fb, &s.meta, sizeof(s.meta));
        footer_append(fb, s.group_rows.data(), s.group_rows.size() * 4);
        for (auto &colnodes : s.nodes) {
            for (auto &nd : colnodes) {
                footer_append(fb, &nd.n, sizeof(nd.n));
                footer_append(fb, nd.segs.data(), nd.segs.size() * sizeof(csf_seg));
            }
        }
    }
    uint64_t foff = w->file_pos;
    if (fwrite(fb.data(), 1, fb.size(), w->f) != fb.size()) { cs_set_err("footer: short write"); cstripe_write_abort(w); return CSTRIPE_ERR_IO; }
    fwrite(&foff, 1, 8, w->f);
    fwrite(CSF_FOOT_MAGIC, 1, 8, w->f);
    int frc = fclose(w->f);
    w->f = nullptr;
    delete w;
    if (frc != 0) { cs_set_err("close failed"); return CSTRIPE_ERR_IO; }
    return CSTRIPE_OK;
}

extern "C" void cstripe_write_abort(cstripe_writer *w)
{
    if (!w) return;
    if (w->f) fclose(w->f);
    delete w;
}

/* ============================ reader ============================ */

/* parse one shard file's footer, appending its stripes (tagged file_idx) */
static int footer_read_one(cstripe_reader *r, uint32_t file_idx)
{
    const cs_file &fl = r->files[file_idx];
    const uint8_t *map = fl.map;
    size_t map_size = fl.map_size;
    if (map_size < CSF_HEADER_SIZE + 16) { cs_set_err("file too small"); return CSTRIPE_ERR_FORMAT; }
    if (memcmp(map, CSF_MAGIC, 8) != 0) { cs_set_err("bad header magic"); return CSTRIPE_ERR_FORMAT; }
    if (memcmp(map + map_size - 8, CSF_FOOT_MAGIC, 8) != 0) { cs_set_err("bad footer magic"); return CSTRIPE_ERR_FORMAT; }
    uint64_t foff;
    memcpy(&foff, map + map_size - 16, 8);
    if (foff + 16 > map_size) { cs_set_err("bad footer offset"); return CSTRIPE_ERR_FORMAT; }

    const uint8_t *p = map + foff;
    const uint8_t *end = map + map_size - 16;
    auto need = [&](size_t n) -> bool { return (size_t)(end - p) >= n; };

    csf_footer_head head;
    if (!need(sizeof(csf_footer_head))) { cs_set_err("truncated footer"); return CSTRIPE_ERR_FORMAT; }
    memcpy(&head, p, sizeof(head));
    p += sizeof(head);
    if (head.version != CSF_VERSION) { cs_set_err("bad version %u", head.version); return CSTRIPE_ERR_FORMAT; }
    if (head.column_count == 0 || head.column_count > 64) { cs_set_err("bad column count"); return CSTRIPE_ERR_FORMAT; }

    std::vector<csf_coldef> cols(head.column_count);
    for (auto &c : cols) {
        if (!need(sizeof(c))) { cs_set_err("truncated coldefs"); return CSTRIPE_ERR_FORMAT; }
        memcpy(&c, p, sizeof(c));
        p += sizeof(c);
    }
    if (file_idx == 0) {
        r->head = head;
        r->cols = cols;
    } else {
        /* shard schema must match (same physical types/widths) */
        if (head.column_count != r->head.column_count) { cs_set_err("shard schema mismatch"); return CSTRIPE_ERR_FORMAT; }
        for (uint32_t i = 0; i < head.column_count; i++)
            if (cols[i].type != r->cols[i].type) { cs_set_err("shard schema mismatch (col %u)", i); return CSTRIPE_ERR_FORMAT; }
        /* scan tiling derives tiles_per_group from file 0's chunk_row_limit;
         * a shard with a larger limit would have rows past that bound
         * silently skipped (round-1 advisor finding) — reject mismatches */
        if (head.chunk_row_limit != r->head.chunk_row_limit) {
            cs_set_err("shard chunk_group_row_limit mismatch (%u vs %u)",
                       head.chunk_row_limit, r->head.chunk_row_limit);
            return CSTRIPE_ERR_FORMAT;
        }
        r->head.total_rows += head.total_rows;
        r->head.stripe_count += head.stripe_count;
    }

    size_t base = r->stripes.size();
    r->stripes.resize(base + head.stripe_count);
    for (size_t si = base; si < r->stripes.size(); si++) {
        auto &s = r->stripes[si];
        s.file_idx = file_idx;
        if (!need(sizeof(s.meta))) { cs_set_err("truncated stripe meta"); return CSTRIPE_ERR_FORMAT; }
        memcpy(&s.meta, p, sizeof(s.meta));
        p += sizeof(s.meta);
        if (s.meta.chunk_count > 1u << 22) { cs_set_err("bad chunk count"); return CSTRIPE_ERR_FORMAT; }
        s.group_rows.resize(s.meta.chunk_count);
        if (!need(s.group_rows.size() * 4)) { cs_set_err("truncated group rows"); return CSTRIPE_ERR_FORMAT; }
        memcpy(s.group_rows.data(), p, s.group_rows.size() * 4);
        p += s.group_rows.size() * 4;
        s.nodes.resize(head.column_count);
        for (auto &cn : s.nodes) {
            cn.resize(s.meta.chunk_count);
            for (auto &nd : cn) {
                if (!need(sizeof(nd.n))) { cs_set_err("truncated skipnode"); return CSTRIPE_ERR_FORMAT; }
                memcpy(&nd.n, p, sizeof(nd.n));
                p += sizeof(nd.n);
                if (nd.n.n_segs == 0 || nd.n.n_segs > 4096) { cs_set_err("bad n_segs"); return CSTRIPE_ERR_FORMAT; }
                nd.segs.resize(nd.n.n_segs);
                if (!need(nd.segs.size() * sizeof(csf_seg))) { cs_set_err("truncated segs"); return CSTRIPE_ERR_FORMAT; }
                memcpy(nd.segs.data(), p, nd.segs.size() * sizeof(csf_seg));
                p += nd.segs.size() * sizeof(csf_seg);
                /* split the packed decomp_len: 24-bit length + stream-shape
                 * mode (format.h); v1 files carry mode 0 = generic */
                nd.seg_modes.resize(nd.segs.size());
                for (size_t si2 = 0; si2 < nd.segs.size(); si2++) {
                    nd.seg_modes[si2] = csf_seg_mode(&nd.segs[si2]);
                    nd.segs[si2].decomp_len &= CSF_SEG_DLEN_MASK;
                }
            }
        }
    }
    return CSTRIPE_OK;
}

static int map_one(cstripe_reader *r, const char *path)
{
    int fd = open(path, O_RDONLY);
    if (fd < 0) { cs_set_err("open %s failed", path); return CSTRIPE_ERR_IO; }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 0) { cs_set_err("stat %s failed", path); close(fd); return CSTRIPE_ERR_IO; }
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) { cs_set_err("mmap %s failed", path); close(fd); return CSTRIPE_ERR_IO; }
    cs_file fl;
    fl.fd = fd;
    fl.map = (const uint8_t *)m;
    fl.map_size = (size_t)st.st_size;
    r->files.push_back(fl);
    return CSTRIPE_OK;
}

/* path may be one stripe file, or a DIRECTORY of shard files (*.cs, sorted
 * by name) scanned as one table — the static shard-group-per-GPU mapping of
 * SURVEY §8e (the reference's shard placements, adaptive_executor.c) */
extern "C" cstripe_reader *cstripe_open(const char *path)
{
    auto *r = new cstripe_reader();
    struct stat st;
    if (stat(path, &st) != 0) { cs_set_err("stat %s failed", path); delete r; return nullptr; }
    if (S_ISDIR(st.st_mode)) {
        DIR *d = opendir(path);
        if (!d) { cs_set_err("opendir %s failed", path); delete r; return nullptr; }
        std::vector<std::string> names;
        struct dirent *de;
        while ((de = readdir(d)) != nullptr) {
            std::string n = de->d_name;
            if (n.size() > 3 && n.substr(n.size() - 3) == ".cs")
                names.push_back(std::string(path) + "/" + n);
        }
        closedir(d);
        std::sort(names.begin(), names.end());
        if (names.empty()) { cs_set_err("no *.cs shard files in %s", path); delete r; return nullptr; }
        for (auto &n : names)
            if (map_one(r, n.c_str()) != CSTRIPE_OK) { cstripe_close(r); return nullptr; }
    } else {
        if (map_one(r, path) != CSTRIPE_OK) { cstripe_close(r); return nullptr; }
    }
    for (uint32_t i = 0; i < r->files.size(); i++)
        if (footer_read_one(r, i) != CSTRIPE_OK) { cstripe_close(r); return nullptr; }
    return r;
}

extern "C" void cstripe_close(cstripe_reader *r)
{
    if (!r) return;
    for (auto &fl : r->files) {
        if (fl.map) munmap((void *)fl.map, fl.map_size);
        if (fl.fd >= 0) close(fl.fd);
    }
    delete r;
}

extern "C" uint64_t cstripe_row_count(const cstripe_reader *r) { return r ? r->head.total_rows : 0; }
extern "C" uint32_t cstripe_column_count(const cstripe_reader *r) { return r ? r->head.column_count : 0; }
extern "C" uint32_t cstripe_stripe_count(const cstripe_reader *r) { return r ? r->head.stripe_count : 0; }

extern "C" int cstripe_column_def(const cstripe_reader *r, uint32_t col, cstripe_coldef *out)
{
    if (!r || col >= r->cols.size() || !out) return CSTRIPE_ERR_ARG;
    memcpy(out->name, r->cols[col].name, 32);
    out->type = r->cols[col].type;
    out->scale = r->cols[col].scale;
    return CSTRIPE_OK;
}

/* ============================ pruning / scan ============================ */

/* range refutation of one predicate against a chunk's [min,max] — the
 * BuildBaseConstraint/UpdateConstraint/predicate_refuted_by combination of
 * SelectedChunkMask (columnar_reader.c:1132-1187) specialized to the
 * pushdownable family. Returns true if NO row in [min,max] can satisfy. */
static bool pred_refutes(const cstripe_pred &p, uint8_t type, int64_t min_i, int64_t max_i,
                         int64_t text_key)
{
    if (type == CSTRIPE_VARTEXT) {
        /* min/max are prefix keys (vartext.h): monotone under memcmp order
         * but not injective, so every bound is the weak one — a chunk whose
         * boundary value shares the constant's 7-byte prefix is kept */
        const int64_t kc = text_key;
        switch (p.op) {
            case CSTRIPE_PRED_LT:
            case CSTRIPE_PRED_LE: return min_i > kc;
            case CSTRIPE_PRED_GT:
            case CSTRIPE_PRED_GE: return max_i < kc;
            case CSTRIPE_PRED_EQ: return kc < min_i || kc > max_i;
            default:              return false;
        }
    }
    if (type == CSTRIPE_F32 || type == CSTRIPE_F64) {
        double mn, mx;
        memcpy(&mn, &min_i, 8);
        memcpy(&mx, &max_i, 8);
        double c = p.fval;
        /* PG float ordering throughout (NaN high, NaN == NaN) — the
         * reference goes through predicate_refuted_by with float8 operator
         * semantics, so e.g. a chunk whose only rows above c are NaN must
         * NOT be pruned for `col > c` (its max IS NaN under this order) */
        switch (p.op) {
            case CSTRIPE_PRED_LT: return f64_cmp_pg(mn, c) >= 0;
            case CSTRIPE_PRED_LE: return f64_cmp_pg(mn, c) > 0;
            case CSTRIPE_PRED_GT: return f64_cmp_pg(mx, c) <= 0;
            case CSTRIPE_PRED_GE: return f64_cmp_pg(mx, c) < 0;
            case CSTRIPE_PRED_EQ: return f64_cmp_pg(c, mn) < 0 || f64_cmp_pg(c, mx) > 0;
            case CSTRIPE_PRED_NE: return f64_cmp_pg(mn, c) == 0 && f64_cmp_pg(mx, c) == 0;
        }
        return false;
    }
    if (type == CSTRIPE_TEXT) {
        /* TEXT min/max hold the C-collation lex key (format.h); EQ/NE are
         * order-independent, so refutation through ANY consistent order is
         * sound — range operators are never refuted (the ABI's row-level
         * text ordering is whole-slot, not collation) */
        const int64_t c = csf_text_lex_key((uint32_t)p.ival);
        switch (p.op) {
            case CSTRIPE_PRED_EQ: return c < min_i || c > max_i;
            case CSTRIPE_PRED_NE: return min_i == c && max_i == c;
            default:              return false;
        }
    }
    int64_t c = p.ival;
    switch (p.op) {
        case CSTRIPE_PRED_LT: return min_i >= c;
        case CSTRIPE_PRED_LE: return min_i > c;
        case CSTRIPE_PRED_GT: return max_i <= c;
        case CSTRIPE_PRED_GE: return max_i < c;
        case CSTRIPE_PRED_EQ: return c < min_i || c > max_i;
        case CSTRIPE_PRED_NE: return min_i == c && max_i == c;
    }
    return false;
}

extern "C" cstripe_scan *cstripe_scan_begin(cstripe_reader *r, uint64_t cols_mask,
                                            const cstripe_pred *preds, uint32_t n_preds)
{
    return cstripe_scan_begin_ex(r, cols_mask, preds, n_preds, nullptr, 0);
}

extern "C" cstripe_scan *cstripe_scan_begin_ex(cstripe_reader *r, uint64_t cols_mask,
                                               const cstripe_pred *preds, uint32_t n_preds,
                                               const cstripe_text_const *text_consts,
                                               uint32_t n_text_consts)
{
    return cstripe_scan_begin_sets(r, cols_mask, preds, n_preds, text_consts, n_text_consts,
                                   nullptr, 0);
}

static inline bool pred_is_set(const cstripe_pred &p)
{
    return p.op == CSTRIPE_PRED_IN || p.op == CSTRIPE_PRED_NOT_IN;
}

/* IN over a sorted key list: true when no key lies in [min, max] */
static bool set_refutes(const std::vector<int64_t> &keys, int64_t min_i, int64_t max_i)
{
    auto it = std::lower_bound(keys.begin(), keys.end(), min_i);
    return it == keys.end() || *it > max_i;
}

extern "C" cstripe_scan *cstripe_scan_begin_sets(cstripe_reader *r, uint64_t cols_mask,
                                                 const cstripe_pred *preds, uint32_t n_preds,
                                                 const cstripe_text_const *text_consts,
                                                 uint32_t n_text_consts,
                                                 const cstripe_value_set *sets, uint32_t n_sets)
{
    return cstripe_scan_begin_lookups(r, cols_mask, preds, n_preds, text_consts, n_text_consts,
                                      sets, n_sets, nullptr, 0);
}

/* validate and copy the lookups of a scan (no device work before every
 * argument check has passed); false with the message set */
static bool lookups_begin(cstripe_scan *s, const cstripe_lookup *lookups, uint32_t n_lookups)
{
    cstripe_reader *r = s->r;
    if (n_lookups > CSTRIPE_MAX_LOOKUPS) { cs_set_err("scan_begin_lookups: %u lookups (max %d)", n_lookups, CSTRIPE_MAX_LOOKUPS); return false; }
    if (n_lookups && !lookups) { cs_set_err("scan_begin_lookups: %u lookups but no array", n_lookups); return false; }
    uint32_t next_col = r->head.column_count;
    s->lookups.resize(n_lookups);
    for (uint32_t l = 0; l < n_lookups; l++) {
        const cstripe_lookup &in = lookups[l];
        cs_lookup &lk = s->lookups[l];
        if (in.n_payloads == 0 || in.n_payloads > CSTRIPE_MAX_LOOKUP_PAYLOADS) {
            cs_set_err("scan_begin_lookups: lookup %u has %u payloads (1..%d)", l, in.n_payloads, CSTRIPE_MAX_LOOKUP_PAYLOADS);
            return false;
        }
        if (in.n > CSTRIPE_MAX_SET_VALUES) {
            cs_set_err("scan_begin_lookups: lookup %u holds %llu entries (max %llu)", l,
                       (unsigned long long)in.n, (unsigned long long)CSTRIPE_MAX_SET_VALUES);
            return false;
        }
        if (in.flags & ~CSTRIPE_LOOKUP_INNER) { cs_set_err("scan_begin_lookups: lookup %u: unknown flags 0x%x", l, in.flags); return false; }
        if (in.n && !in.keys) { cs_set_err("scan_begin_lookups: lookup %u has %llu entries but no keys", l, (unsigned long long)in.n); return false; }
        for (uint32_t p = 0; p < in.n_payloads; p++)
            if (in.n && !in.payloads[p]) {
                cs_set_err("scan_begin_lookups: lookup %u has %llu entries but payload %u is NULL", l, (unsigned long long)in.n, p);
                return false;
            }
        if (in.key_column >= r->head.column_count) {
            cs_set_err("scan_begin_lookups: lookup %u: key column %u out of range", l, in.key_column);
            return false;
        }
        const uint8_t kt = r->cols[in.key_column].type;
        if (kt != CSTRIPE_I8 && kt != CSTRIPE_I16 && kt != CSTRIPE_I32 && kt != CSTRIPE_I64) {
            cs_set_err("scan_begin_lookups: lookup %u: key column %u must be I8/I16/I32/I64", l, in.key_column);
            return false;
        }
        if (next_col + in.n_payloads > 64) {
            cs_set_err("scan_begin_lookups: lookup %u: table plus derived columns exceed 64", l);
            return false;
        }
        lk.key_column = in.key_column;
        lk.n_payloads = in.n_payloads;
        lk.first_col = next_col;
        next_col += in.n_payloads;
        lk.inner = (in.flags & CSTRIPE_LOOKUP_INNER) != 0;
        lk.on_device = in.on_device != 0 && in.n != 0;
        lk.n = in.n;
    }
    s->n_derived = next_col - r->head.column_count;
    /* host maps: copies, duplicate check, ranges */
    for (uint32_t l = 0; l < n_lookups; l++) {
        const cstripe_lookup &in = lookups[l];
        cs_lookup &lk = s->lookups[l];
        if (lk.on_device || !lk.n) continue;
        lk.keys.assign(in.keys, in.keys + in.n);
        lk.sorted_keys = lk.keys;
        std::sort(lk.sorted_keys.begin(), lk.sorted_keys.end());
        for (size_t i = 1; i < lk.sorted_keys.size(); i++)
            if (lk.sorted_keys[i] == lk.sorted_keys[i - 1]) {
                cs_set_err("scan_begin_lookups: lookup %u: duplicate build key %lld (build keys must be distinct)",
                           l, (long long)lk.sorted_keys[i]);
                return false;
            }
        lk.klo = lk.sorted_keys.front();
        lk.khi = lk.sorted_keys.back();
        for (uint32_t p = 0; p < lk.n_payloads; p++) {
            lk.payloads[p].assign(in.payloads[p], in.payloads[p] + in.n);
            const auto mm = std::minmax_element(lk.payloads[p].begin(), lk.payloads[p].end());
            lk.plo[p] = *mm.first;
            lk.phi[p] = *mm.second;
        }
    }
    return true;
}

/* device maps: one reduction launch per array; after every argument check */
static bool lookups_begin_device(cstripe_scan *s, const cstripe_lookup *lookups)
{
    for (size_t l = 0; l < s->lookups.size(); l++) {
        cs_lookup &lk = s->lookups[l];
        if (!lk.on_device) continue;
        const cstripe_lookup &in = lookups[l];
        lk.dev_keys = in.keys;
        if (csgpu_set_range(in.keys, in.n, &lk.klo, &lk.khi, &lk.dev_id) != CSTRIPE_OK) return false;
        for (uint32_t p = 0; p < lk.n_payloads; p++) {
            int dev = -1;
            lk.dev_payloads[p] = in.payloads[p];
            if (csgpu_set_range(in.payloads[p], in.n, &lk.plo[p], &lk.phi[p], &dev) != CSTRIPE_OK) return false;
            if (dev != lk.dev_id) {
                cs_set_err("scan_begin_lookups: lookup %u: payload %u lives on device %d, the keys on device %d",
                           (unsigned)l, p, dev, lk.dev_id);
                return false;
            }
        }
    }
    return true;
}

/* `key_column IN keys` refutation of one lookup over a chunk's [min, max] */
static bool lookup_refutes(const cs_lookup &lk, const csf_skipnode &nd)
{
    if (!nd.has_min_max) return false;
    if (lk.n == 0) return true;
    if (lk.on_device) return lk.khi < nd.min_i || lk.klo > nd.max_i;
    auto it = std::lower_bound(lk.sorted_keys.begin(), lk.sorted_keys.end(), nd.min_i);
    return it == lk.sorted_keys.end() || *it > nd.max_i;
}

extern "C" cstripe_scan *cstripe_scan_begin_lookups(cstripe_reader *r, uint64_t cols_mask,
                                                    const cstripe_pred *preds, uint32_t n_preds,
                                                    const cstripe_text_const *text_consts,
                                                    uint32_t n_text_consts,
                                                    const cstripe_value_set *sets, uint32_t n_sets,
                                                    const cstripe_lookup *lookups, uint32_t n_lookups)
{
    return cstripe_scan_begin_exprs(r, cols_mask, preds, n_preds, text_consts, n_text_consts,
                                    sets, n_sets, lookups, n_lookups, nullptr, 0);
}

/* validate and copy the expressions of a scan, after lookups_begin (their
 * derived columns are legal inputs): one pass per program that simulates the
 * stack depth; false with the message set */
static bool exprs_begin(cstripe_scan *s, const cstripe_expr *exprs, uint32_t n_exprs)
{
    cstripe_reader *r = s->r;
    if (n_exprs > CSTRIPE_MAX_EXPRS) { cs_set_err("scan_begin_exprs: %u expressions (max %d)", n_exprs, CSTRIPE_MAX_EXPRS); return false; }
    if (n_exprs && !exprs) { cs_set_err("scan_begin_exprs: %u expressions but no array", n_exprs); return false; }
    const uint32_t first = r->head.column_count + s->n_derived;
    if (first + n_exprs > 64) {
        cs_set_err("scan_begin_exprs: %u table plus %u derived plus %u computed columns exceed 64",
                   r->head.column_count, s->n_derived, n_exprs);
        return false;
    }
    std::vector<cs_expr> out(n_exprs);
    for (uint32_t e = 0; e < n_exprs; e++) {
        const cstripe_expr &in = exprs[e];
        if (in.n_ops == 0 || in.n_ops > CSTRIPE_MAX_EXPR_OPS || !in.ops) {
            cs_set_err("scan_begin_exprs: expression %u has %u ops (1..%d)", e, in.n_ops, CSTRIPE_MAX_EXPR_OPS);
            return false;
        }
        uint32_t depth = 0;
        for (uint32_t i = 0; i < in.n_ops; i++) {
            const cstripe_expr_op &op = in.ops[i];
            uint32_t pops;
            switch (op.op) {
                case CSTRIPE_EX_COL: case CSTRIPE_EX_CONST: case CSTRIPE_EX_NULL:
                    pops = 0; break;
                case CSTRIPE_EX_NEG: case CSTRIPE_EX_NOT: case CSTRIPE_EX_IS_NULL: case CSTRIPE_EX_YEAR:
                    pops = 1; break;
                case CSTRIPE_EX_SELECT:
                    pops = 3; break;
                default:
                    if (op.op > CSTRIPE_EX_YEAR) {
                        cs_set_err("scan_begin_exprs: expression %u op %u: unknown op %u", e, i, op.op);
                        return false;
                    }
                    pops = 2; break;
            }
            if (op.op == CSTRIPE_EX_COL) {
                if (op.column >= first) {
                    cs_set_err("scan_begin_exprs: expression %u op %u: column %u %s", e, i, op.column,
                               op.column < first + n_exprs
                                   ? "is a computed column (expressions do not chain; nest SELECT)"
                                   : "out of range");
                    return false;
                }
                const uint8_t t = cs_col_type(s, op.column);
                if (t != CSTRIPE_I8 && t != CSTRIPE_I16 && t != CSTRIPE_I32 && t != CSTRIPE_I64) {
                    cs_set_err("scan_begin_exprs: expression %u op %u: column %u must be I8/I16/I32/I64 "
                               "or a lookup-derived column", e, i, op.column);
                    return false;
                }
            }
            if (depth < pops) {
                cs_set_err("scan_begin_exprs: expression %u op %u: stack underflow (op %u needs %u operands, %u on the stack)",
                           e, i, op.op, pops, depth);
                return false;
            }
            depth = depth - pops + 1;
            if (depth > CSTRIPE_MAX_EXPR_DEPTH) {
                cs_set_err("scan_begin_exprs: expression %u op %u: stack depth %u above the limit %d",
                           e, i, depth, CSTRIPE_MAX_EXPR_DEPTH);
                return false;
            }
        }
        if (depth != 1) {
            cs_set_err("scan_begin_exprs: expression %u op %u: the program leaves %u values on the stack, not 1",
                       e, in.n_ops - 1, depth);
            return false;
        }
        out[e].ops.assign(in.ops, in.ops + in.n_ops);
        out[e].first_col = first + e;
    }
    s->exprs = std::move(out);
    /* input columns are read (a derived input has no cols_mask bit) */
    for (const cs_expr &ex : s->exprs)
        for (const cstripe_expr_op &op : ex.ops)
            if (op.op == CSTRIPE_EX_COL && op.column < r->head.column_count)
                s->cols_mask |= 1ull << op.column;
    return true;
}

extern "C" cstripe_scan *cstripe_scan_begin_exprs(cstripe_reader *r, uint64_t cols_mask,
                                                  const cstripe_pred *preds, uint32_t n_preds,
                                                  const cstripe_text_const *text_consts,
                                                  uint32_t n_text_consts,
                                                  const cstripe_value_set *sets, uint32_t n_sets,
                                                  const cstripe_lookup *lookups, uint32_t n_lookups,
                                                  const cstripe_expr *exprs, uint32_t n_exprs)
{
    if (!r) { cs_set_err("scan_begin: null reader"); return nullptr; }
    auto *s = new cstripe_scan();
    s->r = r;
    s->cols_mask = cols_mask;
    if (n_preds > CSTRIPE_MAX_PREDS) { cs_set_err("too many predicates (max %d)", CSTRIPE_MAX_PREDS); delete s; return nullptr; }
    if (!lookups_begin(s, lookups, n_lookups)) { delete s; return nullptr; }
    if (!exprs_begin(s, exprs, n_exprs)) { delete s; return nullptr; }
    s->need_mask = s->cols_mask;   /* the caller's columns and the expressions' inputs */
    {
        uint32_t n_inner = 0;
        for (const cs_lookup &lk : s->lookups) n_inner += lk.inner ? 1 : 0;
        if (n_preds + n_inner > CSTRIPE_MAX_PREDS) {
            cs_set_err("scan_begin_lookups: %u predicates plus %u INNER lookups exceed the %d predicates of one scan",
                       n_preds, n_inner, CSTRIPE_MAX_PREDS);
            delete s; return nullptr;
        }
    }
    /* predicates naming a derived column: checked before any device work */
    for (uint32_t i = 0; i < n_preds; i++) {
        if (preds[i].column < r->head.column_count) continue;
        if (preds[i].column >= cs_scan_ncols(s)) {
            cs_set_err("scan_begin: predicate %u: column %u out of range (%u table + %u derived + %u computed columns)",
                       i, preds[i].column, r->head.column_count, s->n_derived, (unsigned)s->exprs.size());
            delete s; return nullptr;
        }
        if (preds[i].op > CSTRIPE_PRED_NE) {
            cs_set_err("scan_begin_lookups: predicate %u: op %u on %s column %u is not supported "
                       "(LT..NE only; no IN / NOT IN, no LIKE / NOT LIKE)", i, preds[i].op,
                       cs_col_expr(s, preds[i].column) ? "computed" : "derived", preds[i].column);
            delete s; return nullptr;
        }
    }
    if (n_sets > CSTRIPE_MAX_SETS) { cs_set_err("scan_begin_sets: %u value sets (max %d)", n_sets, CSTRIPE_MAX_SETS); delete s; return nullptr; }
    if (n_sets && !sets) { cs_set_err("scan_begin_sets: %u value sets but no array", n_sets); delete s; return nullptr; }
    for (uint32_t i = 0; i < n_text_consts; i++) {
        if (!text_consts || (!text_consts[i].data && text_consts[i].len)) { cs_set_err("scan_begin: text constant %u has no data", i); delete s; return nullptr; }
        s->text_consts.emplace_back((const char *)text_consts[i].data, text_consts[i].len);
    }
    /* the sets: host entries are copied here (integers sorted and
     * deduplicated: the copy chunk refutation searches and the stage
     * uploads); a device set is reduced to its [min, max] */
    s->sets.resize(n_sets);
    for (uint32_t i = 0; i < n_sets; i++) {
        const cstripe_value_set &in = sets[i];
        cs_value_set &vs = s->sets[i];
        if (in.n > CSTRIPE_MAX_SET_VALUES) {
            cs_set_err("scan_begin_sets: set %u holds %llu values (max %llu)", i,
                       (unsigned long long)in.n, (unsigned long long)CSTRIPE_MAX_SET_VALUES);
            delete s; return nullptr;
        }
        if (in.values && in.texts) { cs_set_err("scan_begin_sets: set %u gives both values and texts", i); delete s; return nullptr; }
        if (in.n && !in.values && !in.texts) { cs_set_err("scan_begin_sets: set %u has %llu entries but no data", i, (unsigned long long)in.n); delete s; return nullptr; }
        vs.n = in.n;
        vs.is_text = in.texts != nullptr;
        vs.on_device = in.on_device != 0 && in.values != nullptr;
        if (in.on_device && in.texts) { cs_set_err("scan_begin_sets: set %u: device sets are int64 only", i); delete s; return nullptr; }
        if (vs.is_text) {
            for (uint64_t k = 0; k < in.n; k++) {
                if (!in.texts[k].data && in.texts[k].len) { cs_set_err("scan_begin_sets: set %u text %llu has no data", i, (unsigned long long)k); delete s; return nullptr; }
                vs.texts.emplace_back((const char *)in.texts[k].data, in.texts[k].len);
            }
        } else if (vs.on_device) {
            vs.dev_vals = in.values;
            if (in.n && csgpu_set_range(in.values, in.n, &vs.lo, &vs.hi, &vs.dev_id) != CSTRIPE_OK) { delete s; return nullptr; }
        } else if (in.n) {
            vs.vals.assign(in.values, in.values + in.n);
            std::sort(vs.vals.begin(), vs.vals.end());
            vs.vals.erase(std::unique(vs.vals.begin(), vs.vals.end()), vs.vals.end());
        }
    }
    if (!lookups_begin_device(s, lookups)) { delete s; return nullptr; }
    for (uint32_t i = 0; i < n_preds; i++) {
        if (preds[i].column >= cs_scan_ncols(s)) { cs_set_err("pred column out of range"); delete s; return nullptr; }
        if (cs_col_derived(s, preds[i].column)) {
            /* an ordinary integer atom over a derived (I64) column, checked
             * above; it has no cols_mask bit */
            s->preds.push_back(preds[i]);
            if (s->preds.back().or_group == 0)
                s->preds.back().or_group = 0xFFFFFF00u + i;
            continue;
        }
        if (preds[i].op > CSTRIPE_PRED_NOT_LIKE) { cs_set_err("scan_begin: predicate %u has unknown op %u", i, preds[i].op); delete s; return nullptr; }
        if (cs_pred_is_like(preds[i])) {
            const char *name = preds[i].op == CSTRIPE_PRED_LIKE ? "LIKE" : "NOT LIKE";
            if (r->cols[preds[i].column].type != CSTRIPE_VARTEXT) {
                cs_set_err("scan_begin: predicate %u: op %u (%s) needs a VARTEXT column, column %u "
                           "is not one", i, preds[i].op, name, preds[i].column);
                delete s; return nullptr;
            }
            if (preds[i].ival < 0 || (uint64_t)preds[i].ival >= n_text_consts) {
                cs_set_err("scan_begin: predicate %u is %s: ival %lld is not an index into the "
                           "%u text constants (cstripe_scan_begin_ex)", i, name,
                           (long long)preds[i].ival, n_text_consts);
                delete s; return nullptr;
            }
            const std::string &pat = s->text_consts[(size_t)preds[i].ival];
            const int bad = pat.size() > CSTRIPE_LIKE_MAX_PATTERN ? 1 :
                            cslk_check_pattern((const uint8_t *)pat.data(), (uint32_t)pat.size());
            if (bad) {
                if (bad == 1)
                    cs_set_err("scan_begin: predicate %u: %s pattern of %llu bytes is longer than "
                               "CSTRIPE_LIKE_MAX_PATTERN (%d)", i, name,
                               (unsigned long long)pat.size(), CSTRIPE_LIKE_MAX_PATTERN);
                else if (bad == 2)
                    cs_set_err("scan_begin: predicate %u: LIKE pattern must not end with escape "
                               "character", i);
                else
                    cs_set_err("scan_begin: predicate %u: %s pattern is not valid UTF-8", i, name);
                delete s; return nullptr;
            }
        } else if (pred_is_set(preds[i])) {
            const uint8_t t = r->cols[preds[i].column].type;
            if (preds[i].ival < 0 || (uint64_t)preds[i].ival >= n_sets) {
                cs_set_err("scan_begin: predicate %u is IN / NOT IN: ival %lld is not an index "
                           "into the %u value sets (cstripe_scan_begin_sets)", i,
                           (long long)preds[i].ival, n_sets);
                delete s; return nullptr;
            }
            const cs_value_set &vs = s->sets[(size_t)preds[i].ival];
            if (t == CSTRIPE_F32 || t == CSTRIPE_F64) {
                cs_set_err("scan_begin_sets: predicate %u: IN / NOT IN over float column %u is not supported", i, preds[i].column);
                delete s; return nullptr;
            }
            if (t == CSTRIPE_VARTEXT ? (!vs.is_text && (vs.on_device || sets[preds[i].ival].values))
                                     : vs.is_text) {
                cs_set_err("scan_begin_sets: predicate %u: set %lld gives %s but column %u is %s",
                           i, (long long)preds[i].ival, vs.is_text ? "texts" : "values",
                           preds[i].column, t == CSTRIPE_VARTEXT ? "VARTEXT" : "not VARTEXT");
                delete s; return nullptr;
            }
        } else if (r->cols[preds[i].column].type == CSTRIPE_VARTEXT &&
                   (preds[i].ival < 0 || (uint64_t)preds[i].ival >= n_text_consts)) {
            cs_set_err("scan_begin: predicate %u on VARTEXT column %u needs a string "
                       "constant: ival %lld is not an index into the %u text constants "
                       "(cstripe_scan_begin_ex)", i, preds[i].column,
                       (long long)preds[i].ival, n_text_consts);
            delete s;
            return nullptr;
        }
        s->preds.push_back(preds[i]);
        /* normalize: every predicate belongs to exactly one OR group;
         * standalone conjuncts each get a private id */
        if (s->preds.back().or_group == 0)
            s->preds.back().or_group = 0xFFFFFF00u + i;   /* private ids */
        s->cols_mask |= 1ull << preds[i].column;   /* pred columns must be read */
        if (!cs_pred_is_like(preds[i])) s->need_mask |= 1ull << preds[i].column;
    }
    /* lookups: key columns are read; INNER is the standalone conjunct
     * "derived column 0 IS NOT NULL", the atom GE INT64_MIN */
    for (size_t l = 0; l < s->lookups.size(); l++) {
        const cs_lookup &lk = s->lookups[l];
        s->cols_mask |= 1ull << lk.key_column;
        s->need_mask |= 1ull << lk.key_column;
        if (!lk.inner) continue;
        cstripe_pred q{};
        q.column = lk.first_col;
        q.op = CSTRIPE_PRED_GE;
        q.ival = INT64_MIN;
        q.or_group = 0xFFFFFF00u + n_preds + (uint32_t)l;
        s->preds.push_back(q);
    }
    /* contiguous groups (stable: original order kept within a group) */
    std::stable_sort(s->preds.begin(), s->preds.end(),
                     [](const cstripe_pred &a, const cstripe_pred &b) {
                         return a.or_group < b.or_group;
                     });
    if (s->cols_mask == 0)
        s->cols_mask = s->need_mask = 1;   /* pure count(*): still scan one column's chunks */
    /* chunk-refutation keys of the TEXT / VARTEXT set predicates */
    s->set_keys.resize(s->preds.size());
    bool any_set = false;
    for (size_t i = 0; i < s->preds.size(); i++) {
        const cstripe_pred &p = s->preds[i];
        if (!pred_is_set(p)) continue;
        any_set = true;
        const cs_value_set &vs = s->sets[(size_t)p.ival];
        const uint8_t t = r->cols[p.column].type;
        if (p.op != CSTRIPE_PRED_IN || vs.on_device) continue;
        std::vector<int64_t> &keys = s->set_keys[i];
        if (t == CSTRIPE_TEXT)
            for (int64_t v : vs.vals) keys.push_back(csf_text_lex_key((uint32_t)v));
        else if (t == CSTRIPE_VARTEXT)
            for (const std::string &tx : vs.texts)
                keys.push_back(csvt_prefix_key((const uint8_t *)tx.data(), (uint32_t)tx.size()));
        std::sort(keys.begin(), keys.end());
    }
    /* device pruning (SelectedChunkMask on GPU): same CNF
     * refutation evaluated one-thread-per-chunk; worthwhile when the
     * footer directory holds many thousands of chunk groups. Identical
     * semantics pinned by tests (CSTRIPE_DEVICE_PRUNE=1/0 differential). */
    {
        uint64_t total_chunks = 0;
        for (const auto &st : r->stripes) total_chunks += st.meta.chunk_count;
        const char *dp = getenv("CSTRIPE_DEVICE_PRUNE");
        const int dpv = dp ? atoi(dp) : -1;
        bool any_text = false;   /* TEXT refutation runs host-side (lex-key
                                  * EQ/NE only; kernel not taught the
                                  * transform) */
        for (const auto &p : s->preds)
            any_text |= cs_col_type(s, p.column) == CSTRIPE_TEXT ||
                        cs_col_type(s, p.column) == CSTRIPE_VARTEXT ||
                        cs_col_derived(s, p.column);   /* nor about lookups and expressions */
        any_text |= any_set;     /* nor about value sets */
        std::vector<uint8_t> selmask;
        if (!s->preds.empty() && !any_text && dpv != 0 &&
            (dpv == 1 || total_chunks >= 8192) &&
            csgpu_prune(r, s->preds, selmask) == CSTRIPE_OK &&
            selmask.size() == total_chunks) {
            uint64_t ci = 0;
            for (uint32_t si = 0; si < r->stripes.size(); si++) {
                const cs_stripe_info &st = r->stripes[si];
                for (uint32_t k = 0; k < st.meta.chunk_count; k++, ci++) {
                    if (selmask[ci]) s->sel.push_back({si, k});
                    else s->chunk_groups_filtered++;
                }
            }
            return s;
        }
    }
    for (uint32_t si = 0; si < r->stripes.size(); si++) {
        const cs_stripe_info &st = r->stripes[si];
        for (uint32_t k = 0; k < st.meta.chunk_count; k++) {
            /* chunk removed iff some OR group is WHOLLY refuted — the CNF
             * equivalent of predicate_refuted_by over the reference's
             * AND/OR clause tree (SelectedChunkMask,
             * columnar_reader.c:1132-1187; OR recursion
             * columnar_customscan.c:770-829). Count a removed chunk once. */
            bool selected = true;
            size_t i = 0;
            while (i < s->preds.size() && selected) {
                size_t j = i;
                bool group_refuted = true;
                /* atoms on derived columns: never refuted by value; a group
                 * made only of them, all of ONE lookup, is refuted exactly
                 * when `key_column IN keys` is */
                const cs_lookup *g_lk = nullptr;
                bool g_only_lk = true;
                bool g_expr = false;   /* an atom on a computed column: the group never refutes */
                while (j < s->preds.size() &&
                       s->preds[j].or_group == s->preds[i].or_group) {
                    const cstripe_pred &p = s->preds[j];
                    if (cs_col_expr(s, p.column)) {
                        g_expr = true;
                        j++;
                        continue;
                    }
                    if (cs_col_derived(s, p.column)) {
                        const cs_lookup *lk = cs_col_lookup(s, p.column, nullptr);
                        if (g_lk && g_lk != lk) g_only_lk = false;
                        g_lk = lk;
                        j++;
                        continue;
                    }
                    g_only_lk = false;
                    const csf_skipnode &nd = st.nodes[p.column][k].n;
                    /* all-NULL chunks have no min/max and are never refuted
                     * (columnar_reader.c:1160-1166) */
                    int64_t text_key = 0;
                    if (pred_is_set(p)) {
                        /* IN: no set element in [min, max] (a device set is
                         * known by its range only); NOT IN never refutes */
                        const cs_value_set &vs = s->sets[(size_t)p.ival];
                        const uint8_t t = r->cols[p.column].type;
                        bool refuted = false;
                        if (p.op == CSTRIPE_PRED_IN && nd.has_min_max) {
                            /* a device set's range is over raw values: TEXT
                             * min/max are lex keys, not slots, so there only
                             * the empty set refutes */
                            if (vs.on_device)
                                refuted = vs.n == 0 ||
                                          (t != CSTRIPE_TEXT &&
                                           (vs.hi < nd.min_i || vs.lo > nd.max_i));
                            else
                                refuted = set_refutes(t == CSTRIPE_TEXT || t == CSTRIPE_VARTEXT
                                                          ? s->set_keys[j] : vs.vals,
                                                      nd.min_i, nd.max_i);
                        }
                        if (!refuted) group_refuted = false;
                        j++;
                        continue;
                    }
                    if (cs_pred_is_like(p)) {
                        /* LIKE: every match starts with the pattern's literal
                         * prefix `pre`, so its key lies in [key(pre),
                         * key(pre[:7] padded with 0xFF)]; NOT LIKE never refutes */
                        const std::string &tc = s->text_consts[(size_t)p.ival];
                        uint8_t pre[7];
                        uint32_t np = 0;
                        if (p.op == CSTRIPE_PRED_LIKE && nd.has_min_max)
                            np = cslk_literal_prefix((const uint8_t *)tc.data(), (uint32_t)tc.size(), pre);
                        bool refuted = false;
                        if (np) {
                            const int64_t klo = csvt_prefix_key(pre, np);
                            for (uint32_t b = np; b < 7; b++) pre[b] = 0xFF;
                            const int64_t khi = csvt_prefix_key(pre, 7);
                            refuted = nd.max_i < klo || nd.min_i > khi;
                        }
                        if (!refuted) group_refuted = false;
                        j++;
                        continue;
                    }
                    if (r->cols[p.column].type == CSTRIPE_VARTEXT) {
                        const std::string &tc = s->text_consts[(size_t)p.ival];
                        text_key = csvt_prefix_key((const uint8_t *)tc.data(), (uint32_t)tc.size());
                    }
                    if (!nd.has_min_max ||
                        !pred_refutes(p, r->cols[p.column].type, nd.min_i, nd.max_i, text_key))
                        group_refuted = false;
                    j++;
                }
                if (g_lk)
                    group_refuted = g_only_lk &&
                                    lookup_refutes(*g_lk, st.nodes[g_lk->key_column][k].n);
                if (g_expr) group_refuted = false;
                if (group_refuted) selected = false;
                i = j;
            }
            if (selected) s->sel.push_back({si, k});
            else s->chunk_groups_filtered++;
        }
    }
    return s;
}

extern "C" void cstripe_scan_end(cstripe_scan *s)
{
    if (!s) return;
    csgpu_release(s);
    delete s;
}

extern "C" int64_t cstripe_scan_chunk_groups_filtered(const cstripe_scan *s)
{
    return s ? s->chunk_groups_filtered : 0;
}

extern "C" int cstripe_scan_rewind(cstripe_scan *s)
{
    if (!s) return CSTRIPE_ERR_ARG;
    s->batch_pos = 0;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_last_fused(const cstripe_scan *s) { return s ? s->last_fused : 0; }
extern "C" int cstripe_scan_last_agg_path(const cstripe_scan *s) { return s ? s->last_agg_path : 0; }
extern "C" double cstripe_scan_last_kernel_ms(const cstripe_scan *s) { return s ? s->last_kernel_ms : 0; }
extern "C" double cstripe_scan_last_decode_kernel_ms(const cstripe_scan *s) { return s ? s->last_decode_ms : 0; }
extern "C" double cstripe_scan_last_agg_kernel_ms(const cstripe_scan *s) { return s ? s->last_agg_ms : 0; }

extern "C" int cstripe_gpu_stage(cstripe_scan *s, int device_id)
{
    if (!s) return CSTRIPE_ERR_ARG;
    return csgpu_stage(s, device_id);
}

extern "C" uint64_t cstripe_gpu_staged_bytes(const cstripe_scan *s)
{
    return s ? csgpu_staged_bytes(s) : 0;
}

extern "C" int cstripe_like_match(const uint8_t *pat, uint32_t plen, const uint8_t *val, uint32_t vlen)
{
    if ((!pat && plen) || (!val && vlen)) { cs_set_err("like_match: bad args"); return CSTRIPE_ERR_ARG; }
    const int bad = cslk_check_pattern(pat, plen);
    if (bad) {
        cs_set_err(bad == 1 ? "like_match: pattern longer than CSTRIPE_LIKE_MAX_PATTERN" :
                   bad == 2 ? "LIKE pattern must not end with escape character" :
                              "like_match: pattern is not valid UTF-8");
        return CSTRIPE_ERR_ARG;
    }
    return cslk_match(pat, plen, val, vlen);
}

extern "C" int cstripe_scan_last_like_ms(const cstripe_scan *s, double *match_ms, double *apply_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (match_ms) *match_ms = s->last_like_match_ms;
    if (apply_ms) *apply_ms = s->last_like_apply_ms;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_like_form(const cstripe_scan *s, uint32_t column)
{
    if (!s || !s->gpu || column >= s->like_forms.size()) return CSTRIPE_LIKE_FORM_NONE;
    return s->like_forms[column];
}

extern "C" int cstripe_scan_text_dict(const cstripe_scan *s, uint32_t col, uint32_t *n,
                                      const uint64_t **offsets, const uint8_t **bytes)
{
    if (!s || !n || !offsets || !bytes) { cs_set_err("scan_text_dict: bad args"); return CSTRIPE_ERR_ARG; }
    if (!s->gpu) { cs_set_err("scan not staged — the text dictionary is built by cstripe_gpu_stage"); return CSTRIPE_ERR_NOGPU; }
    if (cstripe_scan_like_form(s, col) == CSTRIPE_LIKE_FORM_STREAM) {
        cs_set_err("scan_text_dict: column %u is only pattern-matched (LIKE stream form) and has "
                   "no dictionary — add it to cols_mask", col);
        return CSTRIPE_ERR_ARG;
    }
    if (col >= s->text_dicts.size() || !s->text_dicts[col].built) {
        cs_set_err("scan_text_dict: column %u is not a projected VARTEXT column", col);
        return CSTRIPE_ERR_ARG;
    }
    const cs_text_dict &d = s->text_dicts[col];
    *n = (uint32_t)(d.offsets.size() - 1);
    *offsets = d.offsets.data();
    *bytes = d.bytes.data();
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_last_set_ms(const cstripe_scan *s, double *build_ms, double *probe_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (build_ms) *build_ms = s->last_set_build_ms;
    if (probe_ms) *probe_ms = s->last_set_probe_ms;
    return CSTRIPE_OK;
}

extern "C" uint32_t cstripe_scan_column_count(const cstripe_scan *s)
{
    return s ? cs_scan_ncols(s) : 0;
}

extern "C" int cstripe_scan_last_lookup_ms(const cstripe_scan *s, double *build_ms, double *probe_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (build_ms) *build_ms = s->last_lookup_build_ms;
    if (probe_ms) *probe_ms = s->last_lookup_probe_ms;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_expr_range(const cstripe_scan *s, uint32_t e, int64_t *lo, int64_t *hi,
                                       uint64_t *n_present)
{
    if (!s || e >= s->exprs.size()) { cs_set_err("scan_expr_range: expression %u is not an expression of this scan", e); return CSTRIPE_ERR_ARG; }
    if (!s->gpu) { cs_set_err("scan_expr_range: scan not staged — the range is measured by cstripe_gpu_stage"); return CSTRIPE_ERR_NOGPU; }
    if (lo) *lo = s->exprs[e].lo;
    if (hi) *hi = s->exprs[e].hi;
    if (n_present) *n_present = s->exprs[e].n_present;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_last_expr_ms(const cstripe_scan *s, double *eval_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (eval_ms) *eval_ms = s->last_expr_ms;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_lookup_form(const cstripe_scan *s, uint32_t lookup_idx, uint64_t *size)
{
    if (!s || lookup_idx >= s->lookups.size()) { cs_set_err("scan_lookup_form: lookup %u is not a lookup of this scan", lookup_idx); return CSTRIPE_ERR_ARG; }
    const bool staged = s->gpu != nullptr;
    if (size) *size = staged ? s->lookups[lookup_idx].form_size : 0;
    return staged ? s->lookups[lookup_idx].form : CSTRIPE_LOOKUP_FORM_NONE;
}

extern "C" int cstripe_scan_set_form(const cstripe_scan *s, uint32_t set_idx, uint64_t *size)
{
    if (!s || set_idx >= s->sets.size()) { cs_set_err("scan_set_form: set %u is not a set of this scan", set_idx); return CSTRIPE_ERR_ARG; }
    const bool staged = s->gpu != nullptr;
    if (size) *size = staged ? s->sets[set_idx].form_size : 0;
    return staged ? s->sets[set_idx].form : CSTRIPE_SET_FORM_NONE;
}

extern "C" int cstripe_scan_last_text_ms(const cstripe_scan *s, double *decode_ms,
                                         double *walk_ms, double *dict_ms, double *remap_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (decode_ms) *decode_ms = s->last_text_decode_ms;
    if (walk_ms) *walk_ms = s->last_text_walk_ms;
    if (dict_ms) *dict_ms = s->last_text_dict_ms;
    if (remap_ms) *remap_ms = s->last_text_remap_ms;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_agg(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                                cstripe_partial *out)
{
    if (!s || !aggs || n_aggs == 0 || !out) { cs_set_err("scan_agg: bad args"); return CSTRIPE_ERR_ARG; }
    return csgpu_agg(s, aggs, n_aggs, nullptr, 0, nullptr, out);
}

extern "C" int cstripe_scan_agg_grouped(cstripe_scan *s, const cstripe_agg_spec *aggs,
                                        uint32_t n_aggs, const uint32_t *group_cols,
                                        uint32_t n_group_cols, cstripe_group_result *gr,
                                        cstripe_partial *out)
{
    if (!s || !aggs || n_aggs == 0 || !out || !gr || n_group_cols == 0 ||
        n_group_cols > CSTRIPE_MAX_GROUP_COLS) { cs_set_err("scan_agg_grouped: bad args"); return CSTRIPE_ERR_ARG; }
    return csgpu_agg(s, aggs, n_aggs, group_cols, n_group_cols, gr, out);
}

extern "C" int cstripe_read_row(cstripe_scan *s, uint64_t row_number,
                                void **col_values, uint8_t *col_nulls)
{
    if (!s || !col_values) { cs_set_err("read_row: bad args"); return CSTRIPE_ERR_ARG; }
    if (!s->preds.empty()) {
        cs_set_err("read_row: random access requires a predicate-free scan "
                   "(the reference's ColumnarReadRowByRowNumber reads with "
                   "empty clause lists)");
        return CSTRIPE_ERR_ARG;
    }
    cstripe_reader *r = s->r;
    for (uint32_t c = 0; c < r->head.column_count; c++)
        if (col_values[c] && r->cols[c].type == CSTRIPE_VARTEXT) {
            cs_set_err("read_row: column %u is VARTEXT — no row access to variable-length "
                       "text; pass NULL for it (scan_select returns dictionary ranks)", c);
            return CSTRIPE_ERR_ARG;
        }
    /* locate the containing selected chunk (scan order = global row order;
     * with no predicates every chunk is selected) */
    if (s->rr_gi < 0 || row_number < s->rr_first ||
        row_number >= s->rr_first + s->rr_rows) {
        uint64_t row_base = 0;
        int64_t gi = -1;
        uint64_t hit_base = 0;
        uint64_t idx = 0;
        for (const auto &sc : s->sel) {
            const cs_stripe_info &st = r->stripes[sc.stripe];
            const uint64_t rows = st.group_rows[sc.chunk];
            if (row_number < row_base + rows) {
                gi = (int64_t)idx;
                hit_base = row_base;
                break;
            }
            row_base += rows;
            idx++;
        }
        if (gi < 0) return CSTRIPE_END;         /* no such row */
        const uint32_t n_cols = r->head.column_count;
        const uint32_t cap = r->head.chunk_row_limit;
        if (s->rr_vals.empty()) {
            s->rr_vals.resize(n_cols);
            s->rr_nulls.resize(n_cols);
            for (uint32_t c = 0; c < n_cols; c++) {
                if (!(s->cols_mask & (1ull << c))) continue;
                s->rr_vals[c].resize((size_t)cap * type_width(r->cols[c].type));
                s->rr_nulls[c].resize(cap);
            }
        }
        std::vector<void *> vp(n_cols, nullptr);
        std::vector<uint8_t *> np(n_cols, nullptr);
        for (uint32_t c = 0; c < n_cols; c++) {
            if (!(s->cols_mask & (1ull << c))) continue;
            if (r->cols[c].type == CSTRIPE_VARTEXT) continue;   /* not readable here */
            vp[c] = s->rr_vals[c].data();
            np[c] = s->rr_nulls[c].data();
        }
        cstripe_batch b{};
        b.col_values = vp.data();
        b.col_nulls = np.data();
        int rc = csgpu_fetch_batch(s, (uint32_t)gi, &b);
        if (rc != CSTRIPE_OK) return rc;
        s->rr_gi = gi;
        s->rr_rows = b.n_rows;
        s->rr_first = hit_base;
    }
    const uint64_t off = row_number - s->rr_first;
    for (uint32_t c = 0; c < r->head.column_count; c++) {
        if (!col_values[c]) continue;
        if (!(s->cols_mask & (1ull << c))) { cs_set_err("read_row: column %u not projected", c); return CSTRIPE_ERR_ARG; }
        const uint32_t w = type_width(r->cols[c].type);
        memcpy(col_values[c], s->rr_vals[c].data() + off * w, w);
        if (col_nulls) col_nulls[c] = s->rr_nulls[c][off];
    }
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_next_batch(cstripe_scan *s, cstripe_batch *batch)
{
    if (!s || !batch) return CSTRIPE_ERR_ARG;
    return csgpu_next_batch(s, batch);
}

extern "C" int cstripe_scan_select_count(cstripe_scan *s, uint64_t *n_rows)
{
    if (!s || !n_rows) { cs_set_err("scan_select_count: bad args"); return CSTRIPE_ERR_ARG; }
    return csgpu_select_count(s, n_rows);
}

extern "C" int cstripe_scan_select(cstripe_scan *s, cstripe_rows *out,
                                   uint64_t capacity, int dst_on_device)
{
    if (!s || !out) { cs_set_err("scan_select: bad args"); return CSTRIPE_ERR_ARG; }
    return csgpu_select(s, out, capacity, dst_on_device);
}

extern "C" int cstripe_scan_last_select_ms(const cstripe_scan *s, double *mask_ms,
                                           double *offsets_ms, double *emit_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (mask_ms) *mask_ms = s->last_select_mask_ms;
    if (offsets_ms) *offsets_ms = s->last_select_offsets_ms;
    if (emit_ms) *emit_ms = s->last_select_emit_ms;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_select_topn(cstripe_scan *s, const cstripe_order_key *order,
                                        uint32_t n_order, uint64_t limit,
                                        cstripe_rows *out, int dst_on_device)
{
    if (!s) { cs_set_err("scan_select_topn: bad args"); return CSTRIPE_ERR_ARG; }
    /* the staged check comes first; argument checks follow it there */
    return csgpu_select_topn(s, order, n_order, limit, out, dst_on_device);
}

extern "C" int cstripe_scan_last_topn_ms(const cstripe_scan *s, double *key_ms,
                                         double *select_ms, double *emit_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (key_ms) *key_ms = s->last_topn_key_ms;
    if (select_ms) *select_ms = s->last_topn_select_ms;
    if (emit_ms) *emit_ms = s->last_topn_emit_ms;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_agg_hashed(cstripe_scan *s, const cstripe_agg_spec *aggs,
                                       uint32_t n_aggs, const uint32_t *key_cols,
                                       uint32_t n_key_cols, uint64_t capacity,
                                       cstripe_hgroups *out)
{
    if (!s) { cs_set_err("scan_agg_hashed: bad args"); return CSTRIPE_ERR_ARG; }
    /* the staged check comes first; argument checks follow it there */
    return csgpu_agg_hashed(s, aggs, n_aggs, key_cols, n_key_cols, capacity, out);
}

extern "C" int cstripe_scan_last_hash_ms(const cstripe_scan *s, double *init_ms,
                                         double *scan_ms, double *compact_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (init_ms) *init_ms = s->last_hash_init_ms;
    if (scan_ms) *scan_ms = s->last_hash_scan_ms;
    if (compact_ms) *compact_ms = s->last_hash_compact_ms;
    return CSTRIPE_OK;
}

extern "C" int cstripe_scan_agg_hashed_topn(cstripe_scan *s,
        const cstripe_agg_spec *aggs, uint32_t n_aggs,
        const uint32_t *key_cols, uint32_t n_key_cols, uint64_t capacity,
        const cstripe_having *having, uint32_t n_having,
        const cstripe_group_order *order, uint32_t n_order,
        uint64_t limit, cstripe_hgroups *out)
{
    if (!s) { cs_set_err("scan_agg_hashed_topn: bad args"); return CSTRIPE_ERR_ARG; }
    /* the staged check comes first; argument checks follow it there */
    return csgpu_agg_hashed_topn(s, aggs, n_aggs, key_cols, n_key_cols, capacity,
                                 having, n_having, order, n_order, limit, out);
}

extern "C" int cstripe_scan_last_group_topn(const cstripe_scan *s, uint64_t *n_groups,
                                            uint64_t *n_kept, double *range_ms,
                                            double *select_ms, double *emit_ms)
{
    if (!s) return CSTRIPE_ERR_ARG;
    if (n_groups) *n_groups = s->last_gt_groups;
    if (n_kept) *n_kept = s->last_gt_kept;
    if (range_ms) *range_ms = s->last_gt_range_ms;
    if (select_ms) *select_ms = s->last_gt_select_ms;
    if (emit_ms) *emit_ms = s->last_gt_emit_ms;
    return CSTRIPE_OK;
}

/* ============================ combine ============================ */

static bool agg_is_count(uint32_t k)
{
    return k == CSTRIPE_AGG_COUNT_STAR || k == CSTRIPE_AGG_COUNT_COL;
}

extern "C" int cagg_combine(const cstripe_agg_spec *aggs, uint32_t n_aggs,
                            const cstripe_partial *parts, uint32_t n_parts,
                            cstripe_partial *out)
{
    if (!aggs || !parts || !out || n_aggs == 0) { cs_set_err("combine: bad args"); return CSTRIPE_ERR_ARG; }
    for (uint32_t a = 0; a < n_aggs; a++) {
        cstripe_partial acc{};
        acc.is_null = 1;
        for (uint32_t p = 0; p < n_parts; p++) {
            const cstripe_partial &in = parts[p * n_aggs + a];
            if (in.is_null) continue;    /* strict combine skips NULL partials
                                          * (aggregate_utils.c:976-1000) */
            if (acc.is_null) { acc = in; continue; }
            switch (aggs[a].kind) {
                case CSTRIPE_AGG_COUNT_STAR:
                case CSTRIPE_AGG_COUNT_COL:
                    acc.count += in.count;
                    acc.i128_lo = acc.count;     /* keep the value mirror consistent */
                    break;
                case CSTRIPE_AGG_SUM_I64:
                case CSTRIPE_AGG_SUM_PROD_I64:
                case CSTRIPE_AGG_SUM_DISC_I64:
                case CSTRIPE_AGG_SUM_DISC_TAX_I64: {
                    __int128 x = ((__int128)acc.i128_hi << 64) | (unsigned long long)acc.i128_lo;
                    __int128 y = ((__int128)in.i128_hi << 64) | (unsigned long long)in.i128_lo;
                    x += y;
                    acc.i128_lo = (int64_t)(uint64_t)x;
                    acc.i128_hi = (int64_t)(x >> 64);
                    acc.count += in.count;
                    break;
                }
                case CSTRIPE_AGG_SUM_F64:
                    acc.f64 += in.f64;
                    acc.count += in.count;
                    break;
                case CSTRIPE_AGG_MIN_I64:
                    acc.i128_lo = std::min(acc.i128_lo, in.i128_lo);
                    acc.i128_hi = acc.i128_lo < 0 ? -1 : 0;
                    acc.count += in.count;
                    break;
                case CSTRIPE_AGG_MAX_I64:
                    acc.i128_lo = std::max(acc.i128_lo, in.i128_lo);
                    acc.i128_hi = acc.i128_lo < 0 ? -1 : 0;
                    acc.count += in.count;
                    break;
                case CSTRIPE_AGG_MIN_F64:
                    if (f64_cmp_pg(in.f64, acc.f64) < 0) acc.f64 = in.f64;
                    acc.count += in.count;
                    break;
                case CSTRIPE_AGG_MAX_F64:
                    if (f64_cmp_pg(in.f64, acc.f64) > 0) acc.f64 = in.f64;
                    acc.count += in.count;
                    break;
                default:
                    cs_set_err("combine: bad agg kind %u", aggs[a].kind);
                    return CSTRIPE_ERR_ARG;
            }
        }
        /* COUNT: NULL -> 0 (COALESCE, multi_logical_optimizer.c:1874-1884) */
        if (acc.is_null && agg_is_count(aggs[a].kind)) {
            acc.is_null = 0;
            acc.count = 0;
        }
        out[a] = acc;
    }
    return CSTRIPE_OK;
}

/* the coordinator merge per group: sort every (part, group) entry by key
 * tuple (NULL keys equal, NULL last), then cagg_combine each run of equal
 * keys — the per-group coord_combine_agg of the reference's grouped plan
 * (aggregate_utils.c:820-1021 under the coordinator's GroupAggregate) */
extern "C" int cagg_combine_groups(const cstripe_agg_spec *aggs, uint32_t n_aggs,
                                   uint32_t n_key_cols, const cstripe_hgroups *parts,
                                   uint32_t n_parts, cstripe_hgroups *out,
                                   uint64_t capacity)
{
    if (!aggs || !out || n_aggs == 0 || (!parts && n_parts > 0) ||
        n_key_cols == 0 || n_key_cols > CSTRIPE_MAX_HASH_KEY_COLS) {
        cs_set_err("combine_groups: bad args");
        return CSTRIPE_ERR_ARG;
    }
    for (uint32_t a = 0; a < n_aggs; a++)
        if (aggs[a].kind > CSTRIPE_AGG_SUM_DISC_TAX_I64) { cs_set_err("combine: bad agg kind %u", aggs[a].kind); return CSTRIPE_ERR_ARG; }
    struct Ent { uint32_t part; uint64_t g; };
    std::vector<Ent> ents;
    for (uint32_t p = 0; p < n_parts; p++) {
        if (parts[p].n_groups == 0) continue;
        if (!parts[p].partials) { cs_set_err("combine_groups: part %u has no partials", p); return CSTRIPE_ERR_ARG; }
        for (uint32_t k = 0; k < n_key_cols; k++)
            if (!parts[p].keys[k] || !parts[p].key_nulls[k]) { cs_set_err("combine_groups: part %u lacks key col %u", p, k); return CSTRIPE_ERR_ARG; }
        for (uint64_t g = 0; g < parts[p].n_groups; g++) ents.push_back({p, g});
    }
    /* <0, 0, >0: signed compare per column, column 0 most significant,
     * NULL last and equal to NULL */
    auto cmp = [&](const Ent &a, const Ent &b) -> int {
        for (uint32_t k = 0; k < n_key_cols; k++) {
            const bool na = parts[a.part].key_nulls[k][a.g] != 0;
            const bool nb = parts[b.part].key_nulls[k][b.g] != 0;
            if (na || nb) {
                if (na && nb) continue;
                return na ? 1 : -1;
            }
            const int64_t va = parts[a.part].keys[k][a.g];
            const int64_t vb = parts[b.part].keys[k][b.g];
            if (va != vb) return va < vb ? -1 : 1;
        }
        return 0;
    };
    std::sort(ents.begin(), ents.end(),
              [&](const Ent &a, const Ent &b) { return cmp(a, b) < 0; });
    uint64_t needed = 0;
    for (size_t i = 0; i < ents.size(); i++)
        if (i == 0 || cmp(ents[i - 1], ents[i]) != 0) needed++;
    if (needed > capacity) {
        out->n_groups = needed;
        cs_set_err("combine_groups: %llu groups > capacity %llu",
                   (unsigned long long)needed, (unsigned long long)capacity);
        return CSTRIPE_ERR_ARG;
    }
    if (needed > 0) {
        if (!out->partials) { cs_set_err("combine_groups: no partials destination"); return CSTRIPE_ERR_ARG; }
        for (uint32_t k = 0; k < n_key_cols; k++)
            if (!out->keys[k] || !out->key_nulls[k]) { cs_set_err("combine_groups: no destination for key col %u", k); return CSTRIPE_ERR_ARG; }
    }
    std::vector<cstripe_partial> run;
    uint64_t og = 0;
    for (size_t i = 0; i < ents.size();) {
        size_t j = i + 1;
        while (j < ents.size() && cmp(ents[i], ents[j]) == 0) j++;
        run.clear();
        for (size_t e = i; e < j; e++) {
            const cstripe_partial *src = parts[ents[e].part].partials + ents[e].g * n_aggs;
            run.insert(run.end(), src, src + n_aggs);
        }
        int rc = cagg_combine(aggs, n_aggs, run.data(), (uint32_t)(j - i),
                              out->partials + og * n_aggs);
        if (rc != CSTRIPE_OK) return rc;
        for (uint32_t k = 0; k < n_key_cols; k++) {
            const bool nul = parts[ents[i].part].key_nulls[k][ents[i].g] != 0;
            out->key_nulls[k][og] = nul ? 1 : 0;
            out->keys[k][og] = nul ? 0 : parts[ents[i].part].keys[k][ents[i].g];
        }
        og++;
        i = j;
    }
    out->n_groups = og;
    return CSTRIPE_OK;
}

/*
 * internal.h — shared host-side structures between cstripe_host.cpp (writer,
 * reader, pruning, combine) and cstripe_gpu.hip (staging + kernels).
 */
#ifndef CSTRIPE_INTERNAL_H
#define CSTRIPE_INTERNAL_H

#include <cstdint>
#include <cstddef>
#include <vector>
#include <string>

#include "../../include/cstripe.h"
#include "format.h"

void cs_set_err(const char *fmt, ...);

struct cs_skipnode {
    csf_skipnode n;
    std::vector<csf_seg> segs;       /* decomp_len MASKED at parse (24-bit) */
    std::vector<uint8_t> seg_modes;  /* CSF_SEGMODE_* per segment */
};

struct cs_stripe_info {
    csf_stripe_meta meta;
    uint32_t file_idx = 0;                       /* which mapped shard file */
    std::vector<uint32_t> group_rows;            /* [chunk] */
    std::vector<std::vector<cs_skipnode>> nodes; /* [col][chunk] */
};

/* one mapped shard file */
struct cs_file {
    int fd = -1;
    const uint8_t *map = nullptr;
    size_t map_size = 0;
};

/* a table = one stripe file OR a directory of shard files (the static
 * shard-group mapping of SURVEY §8e: N shards scanned as one table, one
 * partial out) */
struct cstripe_reader {
    std::vector<cs_file> files;
    csf_footer_head head{};
    std::vector<csf_coldef> cols;
    std::vector<cs_stripe_info> stripes;
    const uint8_t *stripe_base(const cs_stripe_info &st) const
    {
        return files[st.file_idx].map + st.meta.file_offset;
    }
};

struct cs_selchunk {
    uint32_t stripe;
    uint32_t chunk;
};

struct cs_gpu_state;   /* defined in cstripe_gpu.hip */

/* sorted per-scan dictionary of one VARTEXT column (built at stage) */
struct cs_text_dict {
    bool built = false;
    std::vector<uint64_t> offsets;   /* n + 1 */
    std::vector<uint8_t> bytes;      /* entries in memcmp order */
};

/* one value set of IN / NOT_IN predicates (cstripe_scan_begin_sets) */
struct cs_value_set {
    std::vector<int64_t> vals;        /* host integer set: sorted, deduplicated */
    std::vector<std::string> texts;   /* host VARTEXT set, as given */
    bool is_text = false;
    bool on_device = false;
    const int64_t *dev_vals = nullptr;   /* device set: the caller's pointer */
    uint64_t n = 0;                      /* entries as given */
    int dev_id = -1;                     /* device that owns dev_vals */
    int64_t lo = 0, hi = 0;              /* device set: [min, max], n > 0 */
    int form = 0;                        /* CSTRIPE_SET_FORM_* at the last stage */
    uint64_t form_size = 0;              /* slots or bits */
};

/* one lookup (cstripe_scan_begin_lookups): the build side of an N:1 join */
struct cs_lookup {
    uint32_t key_column = 0;
    uint32_t n_payloads = 0;
    uint32_t first_col = 0;              /* column id of payload 0 */
    bool inner = false;
    bool on_device = false;
    uint64_t n = 0;
    std::vector<int64_t> keys;           /* host map: as given (entry order) */
    std::vector<int64_t> sorted_keys;    /* host map: sorted copy (refutation) */
    std::vector<int64_t> payloads[CSTRIPE_MAX_LOOKUP_PAYLOADS];
    const int64_t *dev_keys = nullptr;   /* device map: the caller's pointers */
    const int64_t *dev_payloads[CSTRIPE_MAX_LOOKUP_PAYLOADS] = {};
    int dev_id = -1;                     /* device that owns them */
    int64_t klo = 0, khi = 0;            /* [min, max] of the keys, n > 0 */
    int64_t plo[CSTRIPE_MAX_LOOKUP_PAYLOADS] = {};   /* per payload [min, max] */
    int64_t phi[CSTRIPE_MAX_LOOKUP_PAYLOADS] = {};
    int form = 0;                        /* CSTRIPE_LOOKUP_FORM_* at the last stage */
    uint64_t form_size = 0;
};

/* one expression (cstripe_scan_begin_exprs): a postfix program evaluated at
 * stage into a computed I64 column */
struct cs_expr {
    std::vector<cstripe_expr_op> ops;    /* validated copy of the program */
    uint32_t first_col = 0;              /* its column id */
    int64_t lo = 0, hi = 0;              /* measured at the last stage */
    uint64_t n_present = 0;
};

struct cstripe_scan {
    cstripe_reader *r = nullptr;
    uint64_t cols_mask = 0;
    /* the columns whose VALUES some surface may read: the caller's mask, the
     * expressions' inputs, the lookups' keys and the columns of every
     * predicate but LIKE / NOT LIKE. A VARTEXT column in cols_mask and not
     * here is only pattern-matched (the stage's stream form). */
    uint64_t need_mask = 0;
    std::vector<cstripe_pred> preds;
    std::vector<cs_lookup> lookups;
    uint32_t n_derived = 0;                 /* payload columns of all lookups */
    std::vector<cs_expr> exprs;             /* computed columns, after the derived */
    double last_expr_ms = 0.0;              /* stage-time evaluation launches */
    double last_lookup_build_ms = 0.0;      /* stage-time lookup split */
    double last_lookup_probe_ms = 0.0;
    std::vector<cs_value_set> sets;         /* IN / NOT_IN preds: ival indexes these */
    /* [pred]: sorted chunk-refutation keys of a TEXT (lex keys) or VARTEXT
     * (prefix keys) set predicate; integer columns use sets[].vals */
    std::vector<std::vector<int64_t>> set_keys;
    double last_set_build_ms = 0.0;         /* stage-time set split */
    double last_set_probe_ms = 0.0;
    std::vector<std::string> text_consts;   /* VARTEXT preds: ival indexes these */
    std::vector<cs_text_dict> text_dicts;   /* [column]; built at stage */
    double last_text_decode_ms = 0.0;       /* stage-time VARTEXT split */
    double last_text_walk_ms = 0.0;
    double last_text_dict_ms = 0.0;
    double last_text_remap_ms = 0.0;
    std::vector<uint8_t> like_forms;        /* [column]: CSTRIPE_LIKE_FORM_* at the last stage */
    double last_like_match_ms = 0.0;        /* stage-time LIKE split */
    double last_like_apply_ms = 0.0;
    std::vector<cs_selchunk> sel;     /* surviving chunk groups, scan order */
    int64_t chunk_groups_filtered = 0;
    cs_gpu_state *gpu = nullptr;
    size_t batch_pos = 0;             /* next_batch cursor into sel */
    int last_fused = 0;
    int last_agg_path = 0;            /* CSTRIPE_AGG_PATH_* of the last scan_agg */
    double last_kernel_ms = 0.0;
    double last_decode_ms = 0.0;
    double last_agg_ms = 0.0;
    double last_select_mask_ms = 0.0;     /* scan_select per-kernel split */
    double last_select_offsets_ms = 0.0;
    double last_select_emit_ms = 0.0;
    double last_hash_init_ms = 0.0;       /* scan_agg_hashed per-kernel split */
    double last_hash_scan_ms = 0.0;
    double last_hash_compact_ms = 0.0;
    double last_topn_key_ms = 0.0;        /* scan_select_topn per-stage split */
    double last_topn_select_ms = 0.0;
    double last_topn_emit_ms = 0.0;
    uint64_t last_gt_groups = 0;          /* scan_agg_hashed_topn: groups, kept */
    uint64_t last_gt_kept = 0;
    double last_gt_range_ms = 0.0;        /* and its per-stage split */
    double last_gt_select_ms = 0.0;
    double last_gt_emit_ms = 0.0;
    /* random-access read cache (the reference keeps the current stripe
     * open across ColumnarReadRowByRowNumber calls the same way) */
    int64_t rr_gi = -1;
    std::vector<std::vector<uint8_t>> rr_vals;   /* per col, row-aligned */
    std::vector<std::vector<uint8_t>> rr_nulls;
    uint32_t rr_rows = 0;
    uint64_t rr_first = 0;
};

/* Column addressing of a scan: ids below the table's column count are table
 * columns, the ids after them the derived (lookup payload) columns, then the
 * computed (expression) columns; both kinds are I64 and "derived" here. */
static inline uint32_t cs_scan_ncols(const cstripe_scan *s)
{
    return s->r->head.column_count + s->n_derived + (uint32_t)s->exprs.size();
}
static inline bool cs_pred_is_like(const cstripe_pred &p)
{
    return p.op == CSTRIPE_PRED_LIKE || p.op == CSTRIPE_PRED_NOT_LIKE;
}
static inline bool cs_col_derived(const cstripe_scan *s, uint32_t c)
{
    return c >= s->r->head.column_count && c < cs_scan_ncols(s);
}
/* type of column id c (c < cs_scan_ncols) */
static inline uint8_t cs_col_type(const cstripe_scan *s, uint32_t c)
{
    return c < s->r->head.column_count ? s->r->cols[c].type : (uint8_t)CSTRIPE_I64;
}
/* lookup that owns derived column c; *payload gets its payload index */
static inline const cs_lookup *cs_col_lookup(const cstripe_scan *s, uint32_t c, uint32_t *payload)
{
    for (const cs_lookup &lk : s->lookups)
        if (c >= lk.first_col && c < lk.first_col + lk.n_payloads) {
            if (payload) *payload = c - lk.first_col;
            return &lk;
        }
    return nullptr;
}

/* expression that computes column c, or null */
static inline const cs_expr *cs_col_expr(const cstripe_scan *s, uint32_t c)
{
    const uint32_t first = s->r->head.column_count + s->n_derived;
    return c >= first && c < cs_scan_ncols(s) ? &s->exprs[c - first] : nullptr;
}

/* implemented in cstripe_gpu.hip */
/* device chunk-group pruning (SelectedChunkMask on GPU):
 * evaluates the CNF min/max refutation for every chunk in one launch;
 * selected[global chunk index] = 1 to keep. Returns CSTRIPE_OK, or
 * CSTRIPE_ERR_NOGPU when no device is visible (caller falls back to the
 * host loop). preds must be normalized + group-sorted (scan_begin's form). */
int  csgpu_prune(cstripe_reader *r, const std::vector<cstripe_pred> &preds,
                 std::vector<uint8_t> &selected);
/* [min, max] of a device-resident int64 array (one reduction kernel on the
 * device that owns the pointer, reported in *dev_id); n > 0 */
int  csgpu_set_range(const int64_t *dev_vals, uint64_t n, int64_t *lo, int64_t *hi,
                     int *dev_id);
int  csgpu_stage(cstripe_scan *s, int device_id);
void csgpu_release(cstripe_scan *s);
uint64_t csgpu_staged_bytes(const cstripe_scan *s);
int  csgpu_agg(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
               const uint32_t *group_cols, uint32_t n_group_cols,
               cstripe_group_result *gr, cstripe_partial *out);
int  csgpu_next_batch(cstripe_scan *s, cstripe_batch *batch);
int  csgpu_fetch_batch(cstripe_scan *s, uint32_t gi, cstripe_batch *batch);
/* filtered row materialisation (mask -> offsets -> emit kernels); the mask
 * and bases stay cached on the scan until scan_end / restage */
int  csgpu_select_count(cstripe_scan *s, uint64_t *n_rows);
int  csgpu_select(cstripe_scan *s, cstripe_rows *out, uint64_t capacity,
                  int dst_on_device);
/* hashed GROUP BY (table init -> scan + hash aggregate -> compaction);
 * the device tables hang off the scan and grow on demand */
int  csgpu_agg_hashed(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                      const uint32_t *key_cols, uint32_t n_key_cols,
                      uint64_t capacity, cstripe_hgroups *out);
/* GROUP BY ... HAVING ... ORDER BY ... LIMIT: the front half of
 * csgpu_agg_hashed, then range / HAVING -> keys -> radix select -> gather
 * over the compacted group table; only `limit` groups are copied back */
int  csgpu_agg_hashed_topn(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                           const uint32_t *key_cols, uint32_t n_key_cols,
                           uint64_t capacity, const cstripe_having *having,
                           uint32_t n_having, const cstripe_group_order *order,
                           uint32_t n_order, uint64_t limit, cstripe_hgroups *out);
/* ORDER BY ... LIMIT (key build -> radix select -> refine -> emit ->
 * permute); reads the select cache, writes only its own buffers */
int  csgpu_select_topn(cstripe_scan *s, const cstripe_order_key *order,
                       uint32_t n_order, uint64_t limit, cstripe_rows *out,
                       int dst_on_device);

/* device write path: one chunk's columns compressed on the GPU (canonical
 * parses where the data fits, raw copy-back otherwise) */
struct cs_dev_chunk_col {
    std::vector<uint8_t> data;   /* canonical LZ4 stream, or raw bytes */
    uint8_t mode = 0;            /* CSF_SEGMODE_* when canonical, else 0 */
    int64_t min_i = 0, max_i = 0;
    bool canonical = false;
    bool has_min_max = false;
};
int csgpu_compress_chunk(const void *const *dev_vals, const uint8_t *types,
                         uint32_t n_cols, uint32_t rows, uint64_t row_offset,
                         std::vector<cs_dev_chunk_col> &out);

#endif

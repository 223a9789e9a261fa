/*
 * cstripe.h — C-ABI drop-in boundary for the Citus columnar scan +
 * partial-aggregate hot path, MI355X-native.
 *
 * This header restates, as plain-C POD surfaces, the two reference
 * interfaces the hot path sits behind:
 *
 *  1. Table-AM scan surface:
 *     - cstripe_scan_begin()        mirrors columnar_beginscan_extended()
 *                                   (reference: src/backend/columnar/columnar_tableam.c:205-251)
 *                                   + ColumnarBeginRead (columnar_reader.c:179-239):
 *                                   projection as a column bitmask, quals as
 *                                   pushdownable `Var op const` predicates
 *                                   (columnar_customscan.c:759-952 family).
 *     - cstripe_scan_agg()          the fused whole-scan path replacing the
 *                                   per-row loop under ColumnarScanNext
 *                                   (columnar_customscan.c:1854-1894) +
 *                                   ColumnarReadNextRow (columnar_reader.c:322-361)
 *                                   + the PG Agg transition; one partial
 *                                   accumulator row out, like one worker
 *                                   partial row per shard (multi_logical_optimizer.c:1807-1885).
 *     - cstripe_scan_next_batch()   row/batch fallback access for parity tests,
 *                                   the batch analog of ColumnarReadNextRow
 *                                   (columnar_reader.c:322-361, 868-901).
 *     - cstripe_scan_chunk_groups_filtered() mirrors
 *                                   ColumnarScanChunkGroupsFiltered (columnar_tableam.h:49-60).
 *  2. Combine surface:
 *     - cagg_combine()              reproduces the coordinator merge:
 *                                   coord_combine_agg_sfunc semantics
 *                                   (distributed/utils/aggregate_utils.c:820-1021:
 *                                   strict combine skips null partials, first
 *                                   non-null initializes) and COUNT's NULL->0
 *                                   COALESCE (multi_logical_optimizer.c:1831-1885).
 *
 * Error convention: functions returning int return 0 on success, negative on
 * error; cstripe_errmsg() returns a thread-local message (reference uses
 * ereport(ERROR) longjmp; a C ABI cannot).
 * Threading: one scan = one HIP stream; caller owns batch output buffers.
 *
 * The GPU path REQUIRES a visible MI355X: any cstripe_gpu_* / cstripe_scan_agg
 * call fails loudly (CSTRIPE_ERR_NOGPU) when no HIP device is present. There
 * is no CPU compute fallback in this library; the CPU reference lives in
 * oracle/ (test infrastructure only).
 */
#ifndef CSTRIPE_H
#define CSTRIPE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSTRIPE_ABI_VERSION 2

/* capacity limits of one scan */
#define CSTRIPE_MAX_PREDS 16
#define CSTRIPE_MAX_AGGS  12
/* value sets of one scan (cstripe_scan_begin_sets), and entries of one set */
#define CSTRIPE_MAX_SETS        4
#define CSTRIPE_MAX_SET_VALUES  (1ull << 26)

/* ---- error codes ---- */
#define CSTRIPE_OK            0
#define CSTRIPE_ERR          -1   /* generic; see cstripe_errmsg() */
#define CSTRIPE_ERR_IO       -2
#define CSTRIPE_ERR_FORMAT   -3
#define CSTRIPE_ERR_NOGPU    -4
#define CSTRIPE_ERR_ARG      -5
#define CSTRIPE_END           1   /* scan exhausted (next_batch) */

/* ---- physical column types (fixed-width; by-value in reference terms) ----
 * Serialization follows SerializeSingleDatum (columnar_writer.c:555-585):
 * attlen-sized, att_align_nominal-aligned, packed, PRESENT VALUES ONLY
 * (nulls omitted from the value stream, DeserializeDatumArray
 * columnar_reader.c:1542-1572). For these fixed widths aligned size == width,
 * so a value stream is a dense array of the non-null values. */
typedef enum cstripe_type {
    CSTRIPE_I8  = 1,   /* also categorical char(1) codes ("char"/dictionary byte) */
    CSTRIPE_I16 = 2,
    CSTRIPE_I32 = 3,   /* also date32 (days) */
    CSTRIPE_I64 = 4,   /* also NUMERIC(15,2) as fixed-point int64 (scale in schema) */
    CSTRIPE_F32 = 5,
    CSTRIPE_F64 = 6,
    /* short varlena text (char(1)/bpchar up to 3 payload bytes): each value
     * is stored EXACTLY as the reference serializes a short-form varlena
     * datum — 1-byte header ((total_len << 1) | 1), payload, padded to the
     * 4-byte att_align_nominal boundary (SerializeSingleDatum,
     * columnar_writer.c:555-585; read back by fetch_att/att_addlength_datum,
     * columnar_reader.c:1542-1572). With payload <= 3 every slot is exactly
     * 4 bytes, so the device reads the stream as fixed-stride u32 slots.
     * The ABI passes/returns those raw 4-byte slots; predicates compare
     * whole slots (ival = the constant's slot); GROUP BY keys are the first
     * payload byte (char(1) semantics). */
    CSTRIPE_TEXT = 7,
    /* general variable-length text (the varlena branch of
     * DeserializeDatumArray, columnar_reader.c:1559-1565). The value stream
     * is byte for byte what the reference writes for a text column
     * (SerializeSingleDatum, columnar_writer.c:555-585, typalign 'i'),
     * present values only: a datum whose total length (header + payload) is
     * <= 127 carries the 1-byte short header (total << 1) | 1, any other the
     * 4-byte little-endian header total << 2 (total includes those 4 bytes);
     * each datum is zero-padded to a 4-byte boundary. Payload 0 ..
     * CSTRIPE_VARTEXT_MAX_LEN bytes, no NUL byte. Chunks compress through
     * the generic codec paths; no canonical parse applies.
     *
     * Skip nodes: has_min_max = 1 when any value is present; min_i / max_i
     * hold the PREFIX KEY of the memcmp-smallest / -largest value — its
     * first 7 payload bytes big-endian in bits 55..0, zero-padded: a
     * non-negative int64, monotone under memcmp order, not injective.
     *
     * On the device a VARTEXT column is never read as bytes by the query
     * kernels: cstripe_gpu_stage builds a per-scan sorted dictionary and the
     * column reads as dense int32 RANKS in it (see cstripe_scan_begin_ex). */
    CSTRIPE_VARTEXT = 8,
} cstripe_type;

#define CSTRIPE_VARTEXT_MAX_LEN      65535u
/* most distinct values of one VARTEXT column over the selected chunk groups
 * of one scan; the environment variable CSTRIPE_VARTEXT_MAX_DISTINCT (read
 * per stage) lowers it */
#define CSTRIPE_VARTEXT_MAX_DISTINCT (1u << 20)

/* cstripe_write_rows input of one VARTEXT column: values[c] points at one of
 * these; row i of the batch is bytes[offsets[i] .. offsets[i+1]). A null
 * row's byte range is ignored. */
typedef struct cstripe_vartext_in {
    const uint64_t *offsets;   /* n_rows + 1, non-decreasing */
    const uint8_t  *bytes;
} cstripe_vartext_in;

/* a string constant of a VARTEXT predicate (cstripe_scan_begin_ex) */
typedef struct cstripe_text_const {
    const uint8_t *data;
    uint32_t       len;
} cstripe_text_const;

/* compression codec per column chunk — columnar_compression.c:62-270.
 * Values match the reference's CompressionType enum
 * (columnar_compression.h: NONE=0, PG_LZ=1, LZ4=2, ZSTD=3). */
typedef enum cstripe_compression {
    CSTRIPE_COMP_NONE = 0,
    CSTRIPE_COMP_PGLZ = 1,   /* not produced by this writer; recognized in metadata */
    CSTRIPE_COMP_LZ4  = 2,
    CSTRIPE_COMP_ZSTD = 3,
} cstripe_compression;

/* ---- schema / options ---- */
typedef struct cstripe_coldef {
    char        name[32];
    uint8_t     type;      /* cstripe_type */
    uint8_t     scale;     /* decimal scale for fixed-point int64/int32 (display only) */
    uint8_t     _pad[6];
} cstripe_coldef;

/* knobs mirror columnar GUCs (columnar.c:30-44, :68-120):
 * stripe_row_limit=150000, chunk_group_row_limit=10000, compression, level=3 */
typedef struct cstripe_options {
    uint64_t    stripe_row_limit;      /* default 150000 */
    uint32_t    chunk_group_row_limit; /* default 10000  */
    uint8_t     compression;           /* cstripe_compression, default LZ4 */
    int8_t      compression_level;     /* default 3 (zstd) */
    uint16_t    lz4_seg_target_kb;     /* decompressed KiB per independently
                                        * decodable LZ4 segment (coarse knob;
                                        * one segment == plain whole-chunk
                                        * block, exactly the reference layout) */
    uint32_t    lz4_seg_target_bytes;  /* fine knob, overrides kb when nonzero;
                                        * default 256 B = one GPU lane per
                                        * segment (lane-parallel decode) */
    uint8_t     lz4_min_match;         /* shortest match the writer's LZ4
                                        * encoder emits (>=4; 0 => default).
                                        * Larger = literal-heavier standard-LZ4
                                        * streams that decode faster on GPU at
                                        * a small compression-ratio cost */
    uint8_t     canonical;             /* 1 (default): width-8 chunks whose
                                        * values share their high bytes are
                                        * written as a CANONICAL periodic LZ4
                                        * parse — still a standard block that
                                        * LZ4_decompress_safe decodes — whose
                                        * value positions are closed-form, so
                                        * GPU kernels read values straight
                                        * from the compressed stream with no
                                        * sequence parsing. 0: greedy parse
                                        * everywhere (round-1 behaviour). */
    uint8_t     _pad2[6];
} cstripe_options;

void cstripe_default_options(cstripe_options *opts);

/* ---- predicates ----
 * The family the reference pushes down: `Var op pseudo-const` atoms combined
 * with AND and OR (ExtractPushdownClause, columnar_customscan.c:712-952,
 * OR recursion :770-829). The ABI carries the filter in CNF: predicates
 * sharing a nonzero or_group form one DISJUNCTION; the groups (and all
 * or_group==0 predicates, each its own group) are ANDed. Any AND/OR tree of
 * atoms distributes into this form — e.g. the reference test's
 * `(a>1000 AND a<10000) OR (a>20000 AND a<50000)` becomes the four groups
 * (a>1000 | a>20000)(a>1000 | a<50000)(a<10000 | a>20000)(a<10000 | a<50000)
 * — and chunk refutation over the CNF is equivalent to the reference's
 * predicate_refuted_by on the original tree (a group prunes a chunk only if
 * EVERY member refutes its [min,max]). Trees that exceed CSTRIPE_MAX_PREDS
 * after distribution are not pushdownable through this ABI, mirroring the
 * reference leaving such clauses to ExecQual. Values are given in the
 * column's physical representation (i64 for integer/fixed-point/date
 * columns, f64 for floats). NULL operands fail the atom (SQL semantics at
 * the top-level filter).
 *
 * IN / NOT_IN are the set-membership atoms — `col = ANY(array)`, the
 * ScalarArrayOpExpr the reference pushes into the scan whole, at any list
 * length (columnar_customscan.c:840-850), and `col <> ALL(array)`. Their
 * ival is an INDEX into the value sets of cstripe_scan_begin_sets; one atom
 * whatever the set's size, so a long list does not eat CSTRIPE_MAX_PREDS.
 *
 * LIKE / NOT_LIKE are the pattern atoms over a VARTEXT column; their ival is
 * an INDEX into the text constants of cstripe_scan_begin_ex, which holds the
 * pattern (see "LIKE / NOT LIKE" below cstripe_scan_begin_ex). */
typedef enum cstripe_predop {
    CSTRIPE_PRED_LT = 0, CSTRIPE_PRED_LE, CSTRIPE_PRED_GT, CSTRIPE_PRED_GE,
    CSTRIPE_PRED_EQ, CSTRIPE_PRED_NE,
    CSTRIPE_PRED_IN = 6, CSTRIPE_PRED_NOT_IN = 7,
    CSTRIPE_PRED_LIKE = 8, CSTRIPE_PRED_NOT_LIKE = 9,
} cstripe_predop;

/* longest LIKE pattern, bytes */
#define CSTRIPE_LIKE_MAX_PATTERN 256

typedef struct cstripe_pred {
    uint32_t    column;    /* 0-indexed (reference uses 1-indexed attno) */
    uint32_t    op;        /* cstripe_predop */
    int64_t     ival;      /* comparison constant for integer columns */
    double      fval;      /* comparison constant for float columns */
    uint32_t    or_group;  /* 0 = standalone conjunct; same nonzero id = OR'd */
    uint32_t    _pad;
} cstripe_pred;

/* a value set of IN / NOT_IN predicates (cstripe_scan_begin_sets). A set
 * holds no NULLs; duplicates are allowed. */
typedef struct cstripe_value_set {
    const int64_t            *values;   /* n entries; host memory, or device memory when on_device */
    const cstripe_text_const *texts;    /* n entries, host; for a VARTEXT column (values NULL) */
    uint64_t                  n;        /* 0 is legal */
    uint32_t                  on_device;
    uint32_t                  _pad;
} cstripe_value_set;

/* ---- aggregates ----
 * The worker-partial shapes of the built-ins on the hot path
 * (multi_logical_optimizer.c:1807-1885, :2231-2275, :3279-3308):
 * COUNT -> worker count (int64); SUM/MIN/MAX -> same agg both levels;
 * AVG -> worker (sum, count). Fixed-point NUMERIC sums use int128
 * accumulators (exact). The product forms cover TPC-H Q6/Q1 expressions. */
typedef enum cstripe_aggkind {
    CSTRIPE_AGG_COUNT_STAR = 0,  /* rows passing filter */
    CSTRIPE_AGG_COUNT_COL,       /* non-null values of col a */
    CSTRIPE_AGG_SUM_I64,         /* sum(a)                  -> i128 */
    CSTRIPE_AGG_SUM_F64,         /* sum(a)                  -> f64  */
    CSTRIPE_AGG_MIN_I64, CSTRIPE_AGG_MAX_I64,
    CSTRIPE_AGG_MIN_F64, CSTRIPE_AGG_MAX_F64,
    CSTRIPE_AGG_SUM_PROD_I64,    /* sum(a*b)                -> i128 (Q6 revenue, scale sa+sb) */
    CSTRIPE_AGG_SUM_DISC_I64,    /* sum(a*(ONE-b))          -> i128 (Q1 disc_price) */
    CSTRIPE_AGG_SUM_DISC_TAX_I64,/* sum(a*(ONE-b)*(ONE+c))  -> i128 (Q1 charge) */
} cstripe_aggkind;

typedef struct cstripe_agg_spec {
    uint32_t    kind;            /* cstripe_aggkind */
    int32_t     col_a;           /* -1 for COUNT_STAR */
    int32_t     col_b;           /* product forms */
    int32_t     col_c;           /* disc_tax form */
    int64_t     one;             /* fixed-point ONE for disc/tax forms (100 at scale 2) */
} cstripe_agg_spec;

/* One partial accumulator — the wire shape that replaces a worker partial-agg
 * row (aggregate_utils.c:706-743 serializes transition state per group; ours
 * is the POD equivalent). is_null mirrors a strict transition that saw no
 * rows (aggregate_utils.c:976-1000). */
typedef struct cstripe_partial {
    int64_t     i128_lo;         /* int128 sums: low 64 (two's complement) */
    int64_t     i128_hi;         /*              high 64 */
    double      f64;             /* float sums / min / max */
    int64_t     count;           /* COUNT kinds; also rows contributing */
    uint8_t     is_null;         /* 1 = no rows contributed (strict agg NULL) */
    uint8_t     _pad[7];
} cstripe_partial;

/* ---- group-by (Q1 shape): up to 2 categorical u8/i8 key columns ----
 * NULL keys form their own group, like the reference's HashAggregate
 * (grouping treats NULLs as equal). Key encoding: 9 bits per key column —
 * enc = (value & 0xFF) | (is_null << 8) — packed enc0 | enc1 << 9. */
#define CSTRIPE_MAX_GROUP_COLS 2
#define CSTRIPE_MAX_GROUPS     64
#define CSTRIPE_GROUP_KEY_NULL 0x100u

typedef struct cstripe_group_result {
    uint32_t    n_groups;
    uint32_t    keys[CSTRIPE_MAX_GROUPS];        /* enc0 | enc1<<9 */
    /* partials[g*n_aggs + a] for group g, agg a — caller-provided, size
     * CSTRIPE_MAX_GROUPS * n_aggs */
} cstripe_group_result;

/* ---- batch output (parity/fallback access) ----
 * Caller provides per-column destination arrays (physical width each) and a
 * nulls byte array; the batch is one chunk group (<= chunk_group_row_limit
 * rows), values row-aligned (null slots zero-filled), mirroring
 * ReadChunkGroupNextRow's columnValues/columnNulls contract
 * (columnar_reader.c:868-901) but batched. */
typedef struct cstripe_batch {
    uint32_t    n_rows;          /* out: rows in this batch */
    uint64_t    first_row_number;/* out */
    void      **col_values;      /* in: [n_cols] ptrs, each >= chunk_row_limit*width; unprojected may be NULL */
    uint8_t   **col_nulls;       /* in: [n_cols] ptrs, each >= chunk_row_limit; 1=null */
} cstripe_batch;

/* ---- opaque handles ---- */
typedef struct cstripe_writer cstripe_writer;
typedef struct cstripe_reader cstripe_reader;
typedef struct cstripe_scan   cstripe_scan;

/* =================== writer (format producer; host C) ===================
 * Produces the exact on-disk layout of FlushStripe (columnar_writer.c:391-516):
 * per stripe, per column: all exists streams (bit-packed, SerializeBoolArray
 * :523-545), then all value streams (per-chunk, compressed per
 * SerializeChunkData :592-654 / CompressBuffer, kept raw when incompressible),
 * offsets recorded in skip nodes; skip nodes + chunk-group row counts go to a
 * flat footer directory replacing the columnar.stripe/chunk_group/chunk
 * catalogs (columnar_metadata.c:604-832). */
cstripe_writer *cstripe_write_begin(const char *path, const cstripe_coldef *cols,
                                    uint32_t n_cols, const cstripe_options *opts);
/* column-batch append: n_rows rows; values[c] = array of column c's physical
 * type, row-aligned; nulls[c] may be NULL (all present) else bytes 1=null.
 * A VARTEXT column's values[c] points at a cstripe_vartext_in instead; a
 * value longer than CSTRIPE_VARTEXT_MAX_LEN or holding a NUL byte fails the
 * call with CSTRIPE_ERR_ARG before anything is appended. */
int cstripe_write_rows(cstripe_writer *w, uint64_t n_rows,
                       const void *const *values, const uint8_t *const *nulls);
/* CSTRIPE_OK when exactly n_values VARTEXT datums tile stream[0..len): every
 * datum's header is one of the two forms above, no datum overruns the stream
 * (only the last datum's alignment padding may be missing), and the walk
 * ends after n_values datums, not sooner and not later; CSTRIPE_ERR_FORMAT
 * otherwise. The same header walk runs in the writer's self-check and in the
 * device walk kernel of cstripe_gpu_stage. Host only, no GPU needed. */
int cstripe_vartext_validate(const uint8_t *stream, uint64_t len, uint32_t n_values);
int cstripe_write_end(cstripe_writer *w);     /* flush + footer + close; frees w */
/* device-side append: values[c] are DEVICE pointers to
 * HBM-resident column arrays (query results / ETL). Full chunks are
 * compressed ON the GPU (canonical parses where the data fits; see
 * format.h) so only compressed bytes cross PCIe; other shapes copy back
 * and take the host compressors. Dense rows only — NULL-bearing batches
 * go through cstripe_write_rows. Requires a visible MI355X. A schema with
 * a VARTEXT column returns CSTRIPE_ERR_ARG (checked before the device). */
int cstripe_write_rows_device(cstripe_writer *w, uint64_t n_rows,
                              const void *const *dev_values);
void cstripe_write_abort(cstripe_writer *w);

/* =================== reader / scan =================== */
cstripe_reader *cstripe_open(const char *path);          /* mmap + parse footer */
void cstripe_close(cstripe_reader *r);
uint64_t cstripe_row_count(const cstripe_reader *r);
uint32_t cstripe_column_count(const cstripe_reader *r);
uint32_t cstripe_stripe_count(const cstripe_reader *r);
int cstripe_column_def(const cstripe_reader *r, uint32_t col, cstripe_coldef *out);

/* scan_begin: projection as a bitmask over columns (bit c = column c needed),
 * preds implicitly ANDed. Performs chunk-group min/max pruning host-side
 * (SelectedChunkMask semantics, columnar_reader.c:1132-1187: a chunk survives
 * unless some predicate refutes its [min,max]; chunks with no min/max always
 * survive). */
cstripe_scan *cstripe_scan_begin(cstripe_reader *r, uint64_t cols_mask,
                                 const cstripe_pred *preds, uint32_t n_preds);
/* scan_begin_ex: scan_begin plus string constants for VARTEXT predicates.
 * For a predicate on a VARTEXT column, ival is an INDEX into text_consts
 * (copied; the caller's memory is not kept). An index >= n_text_consts
 * returns NULL with an error; cstripe_scan_begin fails the same way on any
 * VARTEXT predicate, having no constant to compare against.
 *  - Row semantics: all six operators compare by memcmp order, the shorter
 *    string first on a prefix tie (PG "C" collation); a NULL operand fails
 *    the atom; OR groups as for every type.
 *  - Chunk refutation (host side; the device prune kernel is skipped when a
 *    VARTEXT predicate is present, as for TEXT) works on prefix keys, kc =
 *    key(constant): LT/LE refute when min_key > kc, GT/GE when max_key < kc,
 *    EQ when kc < min_key or kc > max_key, NE never. Keys are monotone but
 *    not injective, so a value sharing its 7-byte prefix with a chunk
 *    boundary never prunes that chunk. All-NULL chunks (no min/max) survive.
 *  - Device evaluation: cstripe_gpu_stage builds, per projected VARTEXT
 *    column, a dictionary of the distinct values of the SELECTED chunk
 *    groups — decode, header walk, a device open-addressing table claimed by
 *    atomicCAS, one gather + one DtoH copy, a host memcmp sort — and rewrites
 *    the column as int32 ranks in that sorted dictionary. Ranks follow
 *    memcmp order, so each predicate becomes one integer atom over ranks
 *    (lb = entries < c, ub = entries <= c): EQ rank == rank(c), or == -1
 *    when c is absent; NE the negation; LT rank < lb; LE rank < ub; GE
 *    rank > lb - 1; GT rank > ub - 1. Every query kernel then treats the
 *    column as a dense I32 column.
 *  - Limits: more than CSTRIPE_VARTEXT_MAX_DISTINCT distinct values (or the
 *    lower CSTRIPE_VARTEXT_MAX_DISTINCT environment value) makes
 *    cstripe_gpu_stage return CSTRIPE_ERR_ARG naming the column and the
 *    limit, and leaves the scan unstaged — a "not pushdownable" domain, like
 *    an over-wide hash key. A malformed stream (a datum that overruns its
 *    chunk, or a datum count other than n_present) makes it return
 *    CSTRIPE_ERR_FORMAT; the walk is bounded by decompressed_size, so this
 *    is a flag, never an out-of-range read.
 *  - Ranks are PER SCAN: the dictionary covers the selected chunk groups of
 *    this scan (all files of a shard directory), and a restage rebuilds it.
 *    Ranks of two scans are not comparable, so cagg_combine_groups across
 *    scans with text keys needs a common coding and is not supported.
 *  - What each surface does with a VARTEXT column: predicate column in
 *    scan_agg / scan_agg_grouped / scan_agg_hashed / scan_select — works;
 *    aggregate operand — COUNT_COL only, else CSTRIPE_ERR_ARG; scan_select —
 *    col_values[c] receives int32 ranks (capacity * 4 bytes; NULL gives 0
 *    plus a null byte), host or device destination; scan_agg_hashed key —
 *    allowed, key range [0, n_dict - 1], keys[k][g] is the rank, NULL keys
 *    last, so groups come out in the strings' memcmp order; scan_agg_grouped
 *    key — CSTRIPE_ERR_ARG (use the hashed form); next_batch / read_row —
 *    CSTRIPE_ERR_ARG when that column's destination is non-NULL, the other
 *    columns work when it is NULL. */
cstripe_scan *cstripe_scan_begin_ex(cstripe_reader *r, uint64_t cols_mask,
                                    const cstripe_pred *preds, uint32_t n_preds,
                                    const cstripe_text_const *text_consts,
                                    uint32_t n_text_consts);
/* LIKE / NOT LIKE — CSTRIPE_PRED_LIKE / CSTRIPE_PRED_NOT_LIKE, accepted by
 * cstripe_scan_begin_ex, _sets, _lookups and _exprs on a VARTEXT table
 * column; ival indexes text_consts (the pattern), fval is ignored, or_group
 * works as for every atom. Plain cstripe_scan_begin has no constants and
 * fails.
 *  - Pattern language: PG LIKE with the default escape under "C" collation in
 *    a UTF-8 database. '%' matches any run of characters, none included; '_'
 *    exactly one character; '\x' the byte x literally; any other byte itself.
 *    A character is one byte plus the continuation bytes ((b & 0xC0) == 0x80)
 *    that follow it. The match is anchored at both ends. x LIKE p passes iff
 *    x is non-NULL and matches; x NOT LIKE p iff x is non-NULL and does not;
 *    a NULL operand fails both.
 *  - Exact for patterns and values that are valid UTF-8, pure ASCII included.
 *    For a value that is not valid UTF-8 the verdict is unspecified (PG's
 *    recursive matcher and this one differ on such bytes); it is still
 *    deterministic, terminates, and reads nothing outside the value.
 *  - Begin errors (NULL, the message names the predicate index): the column
 *    is not VARTEXT (TEXT slots, derived and computed ids included); the
 *    constant index is out of range; the pattern is longer than
 *    CSTRIPE_LIKE_MAX_PATTERN; it ends in an unescaped backslash ("LIKE
 *    pattern must not end with escape character"); it is not valid UTF-8.
 *  - Chunk refutation (host): with `pre` the literal bytes before the first
 *    unescaped '%' or '_', escapes resolved — LIKE refutes a chunk that has
 *    min/max iff pre is non-empty and max_key < key(pre) or min_key >
 *    key(pre[:7] padded with 0xFF to 7 bytes). NOT LIKE never refutes;
 *    all-NULL chunks survive; an or_group refutes only if every member does.
 *    The device prune kernel stays off, as for every VARTEXT predicate.
 *  - Device evaluation, at cstripe_gpu_stage: each distinct (column, pattern
 *    bytes) pair becomes one I8 membership column, laid out and counted
 *    exactly like the member slot of an IN / NOT IN pair (one of the 16
 *    projected slots; over the limit the stage returns CSTRIPE_ERR_ARG and
 *    the scan stays unstaged). LIKE is member == 1, NOT LIKE member == 0;
 *    both of one pattern share the slot. No query kernel knows about LIKE.
 *  - Two read forms per column, chosen per stage (cstripe_scan_like_form).
 *    DICT: the column also needs ranks — it is in the caller's cols_mask, or
 *    carries any other predicate or set — so the dictionary is built as
 *    usual, each of its n_dict entries is matched once, and one pass writes
 *    member[i] = flag[slot of value i]. STREAM: the column is absent from the
 *    caller's cols_mask and every predicate on it is LIKE / NOT LIKE —
 *    decode, header walk, then one match per value straight off the walk's
 *    (offset, length) words: no hash table, no gather, no host sort, no
 *    ranks, and no CSTRIPE_VARTEXT_MAX_DISTINCT limit, so a near-unique
 *    comment column can be filtered.
 *  - A STREAM column has no values for anyone else: cstripe_scan_text_dict,
 *    a wanted or order column of scan_select / scan_select_topn, a key of
 *    scan_agg_hashed / scan_agg_hashed_topn and a COUNT_COL operand
 *    return CSTRIPE_ERR_ARG with a message that names the column and says
 *    "add it to cols_mask".
 *  - CSTRIPE_LIKE_FORM=dict|stream (environment, read per stage) is a switch
 *    for tests: `stream` on a column that needs ranks falls back to DICT,
 *    `dict` always works and is subject to the distinct limit. Results never
 *    depend on it.
 *  - Out of scope: ILIKE, SIMILAR TO, regular expressions, a custom ESCAPE
 *    character; LIKE on TEXT slots or inside expressions; LIKE-specific
 *    handling in the device prune kernel; splitting long values across lanes
 *    (one lane matches one value, so lanes diverge on value length);
 *    collations other than "C". */
/* The matcher itself, host only (no GPU needed): 1 when val[0..vlen) matches
 * pat[0..plen), 0 when not, CSTRIPE_ERR_ARG for a pattern scan_begin would
 * refuse. It runs the same source the device match kernel runs (like.h). */
int cstripe_like_match(const uint8_t *pat, uint32_t plen, const uint8_t *val, uint32_t vlen);
/* device milliseconds of the last cstripe_gpu_stage's LIKE work, all
 * patterns together: the match kernels, and the DICT form's apply passes.
 * Both 0 without a LIKE atom. Either out pointer may be NULL. */
int cstripe_scan_last_like_ms(const cstripe_scan *s, double *match_ms, double *apply_ms);
/* read form of table column `column` at the last stage: CSTRIPE_LIKE_FORM_NONE
 * when the scan is unstaged or no LIKE atom names the column */
#define CSTRIPE_LIKE_FORM_NONE   0
#define CSTRIPE_LIKE_FORM_DICT   1
#define CSTRIPE_LIKE_FORM_STREAM 2
int cstripe_scan_like_form(const cstripe_scan *s, uint32_t column);
/* scan_begin_sets: scan_begin_ex plus value sets for IN / NOT_IN atoms. With
 * n_sets == 0 it is exactly cstripe_scan_begin_ex (which calls it).
 *  - For op IN / NOT_IN, ival is an INDEX into sets — for every column type,
 *    VARTEXT included; fval is ignored. Several predicates may name one set.
 *    cstripe_scan_begin and cstripe_scan_begin_ex have no sets and fail on
 *    either op, naming this entry.
 *  - Key column types: I8/I16/I32/I64 — set values are int64, a value outside
 *    the column's range simply never matches; TEXT — values are whole 4-byte
 *    slots zero-extended, as for EQ; VARTEXT — the set gives `texts` (values
 *    NULL): at stage each string is looked up in the column's per-scan
 *    dictionary, absent strings drop out and the set becomes a set of ranks.
 *    An F32/F64 key column returns NULL with a message.
 *  - Memory: host values / texts are copied at begin. A device set
 *    (on_device != 0, int64 only) is read in place: the pointer must stay
 *    valid and unchanged until cstripe_scan_end, because every stage rebuilds
 *    from it. It must live on the device the scan is staged on.
 *  - Row semantics, as in SQL: x IN S passes iff x is non-NULL and in S;
 *    x NOT IN S passes iff x is non-NULL and not in S; a NULL operand fails
 *    either atom. The empty set gives IN -> no row, NOT IN -> every non-NULL
 *    row. Both are ordinary atoms, usable inside an or_group.
 *  - Errors (NULL, message set): a set index >= n_sets, n_sets >
 *    CSTRIPE_MAX_SETS, n > CSTRIPE_MAX_SET_VALUES, texts on a non-VARTEXT
 *    column or values on a VARTEXT column, a device text set, an op above 7.
 *  - Chunk refutation (host side; the device prune kernel is skipped when a
 *    set predicate is present, as for TEXT): IN refutes a chunk that has
 *    min/max iff no set element lies in [min, max] — over the values for
 *    integer columns, over the C-collation lex keys of the slots for TEXT,
 *    over the 7-byte prefix keys for VARTEXT (inclusive bounds, so an element
 *    sharing its prefix with a chunk boundary keeps that chunk). For a device
 *    set one reduction kernel at begin yields the set's [min, max] and
 *    nothing else; IN then refutes only when that range misses the chunk's.
 *    On a TEXT column a device set never refutes (unless empty): its range
 *    is over slot values, the skip nodes hold lex keys.
 *    NOT_IN never refutes. All-NULL chunks (no min/max) survive.
 *  - Device evaluation: all at cstripe_gpu_stage, no query kernel knows about
 *    sets. Each distinct (column, set) pair gets one extra projected slot — a
 *    one-byte MEMBERSHIP column in scratch, sharing the key column's exists
 *    bitmap. A build kernel turns the set into a bitmap over [lo, hi] (when
 *    hi - lo + 1 <= max(2^16, 128 n) and <= 2^32) or an open-addressing hash
 *    table of max(2, next_pow2(2 n)) 64-bit slots; a probe kernel walks the
 *    key column's value streams once and writes 0/1 bytes. IN is then the
 *    integer atom member == 1, NOT_IN member == 0, on every surface
 *    (scan_agg and its grouped / hashed forms, scan_select, select_topn).
 *    Such scans never take the fused or overlapped aggregate bodies
 *    (cstripe_scan_last_agg_path reports DENSE or GENERAL). The slots count
 *    against the 16 projected columns of one scan; overflow is
 *    CSTRIPE_ERR_ARG from cstripe_gpu_stage and leaves the scan unstaged.
 *  - CSTRIPE_SET_FORM=hash|bitmap (environment, read per stage) forces the
 *    form; a forced bitmap over a range beyond 2^32 falls back to hash.
 *    Results never depend on it. */
cstripe_scan *cstripe_scan_begin_sets(cstripe_reader *r, uint64_t cols_mask,
                                      const cstripe_pred *preds, uint32_t n_preds,
                                      const cstripe_text_const *text_consts,
                                      uint32_t n_text_consts,
                                      const cstripe_value_set *sets, uint32_t n_sets);
/* device time (hipEvents, milliseconds) of the last cstripe_gpu_stage's set
 * work, all sets together: table build (clearing the table + the insert
 * kernel; a host set's upload is not in it), membership probe. Both 0 when
 * the scan has no set predicate. Any out pointer may be NULL. */
int cstripe_scan_last_set_ms(const cstripe_scan *s, double *build_ms, double *probe_ms);
/* form chosen for set set_idx at the last stage: 0 none / unstaged / unused,
 * 1 hash, 2 bitmap; *size (may be NULL) gets the table's slots or bits. A
 * set used on several VARTEXT columns reports the last table built from it.
 * CSTRIPE_ERR_ARG when set_idx is not a set of this scan. */
#define CSTRIPE_SET_FORM_NONE   0
#define CSTRIPE_SET_FORM_HASH   1
#define CSTRIPE_SET_FORM_BITMAP 2
int cstripe_scan_set_form(const cstripe_scan *s, uint32_t set_idx, uint64_t *size);

/* ---- lookups: the device N:1 join with payload columns ----
 * A lookup joins the scanned table to a build side (key -> payload values)
 * as a LEFT JOIN whose build keys are distinct: the FK -> PK joins a
 * co-located or reference-table plan pushes to every worker. Each payload
 * becomes a DERIVED COLUMN of the scan that every query surface addresses by
 * a column id past the table's own. */
#define CSTRIPE_MAX_LOOKUPS          2
#define CSTRIPE_MAX_LOOKUP_PAYLOADS  4
#define CSTRIPE_LOOKUP_INNER         1u   /* flags: drop rows without a match */

typedef struct cstripe_lookup {
    uint32_t        key_column;   /* I8/I16/I32/I64 column of the scanned table */
    uint32_t        n_payloads;   /* 1..CSTRIPE_MAX_LOOKUP_PAYLOADS */
    const int64_t  *keys;         /* n build keys, all distinct, no NULLs */
    const int64_t  *payloads[CSTRIPE_MAX_LOOKUP_PAYLOADS];  /* n entries each, parallel to keys */
    uint64_t        n;            /* 0 legal; <= CSTRIPE_MAX_SET_VALUES */
    uint32_t        on_device;    /* keys AND payloads are device memory, read in place */
    uint32_t        flags;        /* CSTRIPE_LOOKUP_* */
} cstripe_lookup;

/* scan_begin_lookups: scan_begin_sets plus lookups. With n_lookups == 0 it is
 * exactly cstripe_scan_begin_sets (which calls it).
 *  - Derived columns: payload p of lookup l is column
 *    cstripe_column_count(r) + (payloads of the lookups before l) + p, type
 *    I64. It is always projected (it has no cols_mask bit) and takes one of
 *    the 16 projected slots of a scan; overflow is CSTRIPE_ERR_ARG from
 *    cstripe_gpu_stage and leaves the scan unstaged. Table plus derived
 *    columns must stay <= 64. The key column is projected implicitly.
 *  - Row semantics: derived column d of a row is payload[e] when the row's key
 *    is non-NULL and equals build key e; NULL otherwise. A key value outside
 *    an I8/I16/I32 key column's range never matches. CSTRIPE_LOOKUP_INNER adds
 *    one standalone conjunct "derived column 0 of this lookup IS NOT NULL"
 *    (the atom GE INT64_MIN); it counts against CSTRIPE_MAX_PREDS.
 *  - A derived id is accepted as the predicate column of LT..NE (a NULL
 *    operand fails the atom, so a standalone predicate on a derived column
 *    gives inner-join semantics), as the operand of COUNT_COL and every I64
 *    aggregate kind, as a cstripe_scan_agg_hashed key, as a
 *    cstripe_scan_select_topn order column, and as a wanted column of
 *    cstripe_scan_select / _select_topn: for a scan with lookups the
 *    per-column arrays of cstripe_rows have cstripe_scan_column_count(s)
 *    entries. Not accepted (CSTRIPE_ERR_ARG / NULL, message set): IN / NOT_IN
 *    on a derived column, cstripe_scan_agg_grouped keys, a TEXT / VARTEXT /
 *    float key column. cstripe_scan_next_batch and cstripe_read_row do not
 *    know derived columns; their arrays stay cstripe_column_count(r) long.
 *  - Key packing (hashed GROUP BY, top-N): a derived column's [lo, hi] is the
 *    [min, max] of its payload array, computed at begin (one reduction launch
 *    per device array). A value outside it is a device array that changed
 *    after begin: the call fails with CSTRIPE_ERR_FORMAT.
 *  - Memory: host arrays are copied at begin. Device arrays (on_device != 0)
 *    are read in place at every stage and must stay valid until
 *    cstripe_scan_end, on the device the scan is staged on (else
 *    CSTRIPE_ERR_ARG at stage). The keys must not change; payload values may
 *    change between stages within their begin-time range.
 *  - Errors at begin (NULL, message set): n_lookups > CSTRIPE_MAX_LOOKUPS,
 *    n_payloads 0 or > 4, a NULL array with n > 0, n above the limit, a bad
 *    key column or key type, a predicate naming a column beyond
 *    cstripe_scan_column_count, too many predicates with the INNER atoms, and
 *    duplicate build keys in a host map (the message names the key).
 *    Duplicates in a device map are found by the build kernel at stage:
 *    cstripe_gpu_stage returns CSTRIPE_ERR_ARG naming the lookup and the scan
 *    stays unstaged.
 *  - Chunk refutation (host loop; the device prune kernel is skipped when a
 *    predicate names a derived column): an atom on a derived column never
 *    refutes by value. An or_group whose members are all atoms on derived
 *    columns of ONE lookup refutes a chunk exactly when `key_column IN keys`
 *    would: for a host map no build key lies in the key column's [min, max];
 *    for a device map the key range misses it. Mixed with other columns it
 *    never refutes. All-NULL key chunks (no min/max) survive.
 *  - Device evaluation: all at cstripe_gpu_stage, after the value sets; no
 *    query kernel knows about lookups. One table per lookup maps key -> entry
 *    index: a direct u32 array over [lo, hi] when hi - lo + 1 <=
 *    max(2^16, 4 n) and < 2^32, else an open-addressing hash table of
 *    max(2, next_pow2(2 n)) slots. A probe kernel writes each derived
 *    column's exists bitmap, a scan kernel its rank table, a gather kernel
 *    its compacted values; the column then reads as an ordinary sparse I64
 *    column in scratch. Such scans report CSTRIPE_AGG_PATH_GENERAL.
 *    CSTRIPE_LOOKUP_FORM=hash|direct (environment, read per stage) forces the
 *    form; a forced direct over an illegal range falls back to hash. Results
 *    never depend on it. It is a switch for tests and measurements: a forced
 *    direct table takes 4 B per value of [lo, hi], whatever n is.
 *    Probe, rank scan and gather run over batches of chunk groups of at most
 *    2^26 rows (CSTRIPE_LOOKUP_BATCH_ROWS overrides it), which bounds the
 *    stage's temporary memory at 256 MB plus the uploaded copy of a host map.
 *  - Out of scope: float / TEXT / VARTEXT payloads and keys, N:M joins
 *    (duplicate build keys), composite keys, derived columns in next_batch /
 *    read_row, a dense fast path when every row matches, exact device-side
 *    pruning for device maps, multi-GPU distribution of the build side. */
cstripe_scan *cstripe_scan_begin_lookups(cstripe_reader *r, uint64_t cols_mask,
                                         const cstripe_pred *preds, uint32_t n_preds,
                                         const cstripe_text_const *text_consts,
                                         uint32_t n_text_consts,
                                         const cstripe_value_set *sets, uint32_t n_sets,
                                         const cstripe_lookup *lookups, uint32_t n_lookups);
/* table columns + derived columns of the scan */
uint32_t cstripe_scan_column_count(const cstripe_scan *s);
/* device time (hipEvents, milliseconds) of the last cstripe_gpu_stage's lookup
 * work, all lookups together: table build (clear + insert kernel; a host
 * map's upload is not in it), probe (bitmap, rank scan, gather). Both 0
 * without a lookup. Any out pointer may be NULL. */
int cstripe_scan_last_lookup_ms(const cstripe_scan *s, double *build_ms, double *probe_ms);
/* form of lookup lookup_idx's table at the last stage: 0 none / unstaged,
 * 1 hash, 2 direct; *size (may be NULL) gets its slots or entries.
 * CSTRIPE_ERR_ARG when lookup_idx is not a lookup of this scan. */
#define CSTRIPE_LOOKUP_FORM_NONE   0
#define CSTRIPE_LOOKUP_FORM_HASH   1
#define CSTRIPE_LOOKUP_FORM_DIRECT 2
int cstripe_scan_lookup_form(const cstripe_scan *s, uint32_t lookup_idx, uint64_t *size);

/* ---- expressions: device-computed columns ----
 * The row-level expressions the reference evaluates in ExecQual / ExecProject
 * over the rows ColumnarScanNext returns (columnar_customscan.c:1854-1913):
 * column-versus-column comparisons, CASE inside an aggregate, arithmetic,
 * extract(year). An expression is a small POSTFIX program over int64 values;
 * cstripe_gpu_stage evaluates it once per row of the selected chunk groups
 * and the result is a COMPUTED COLUMN every query surface addresses by a
 * column id past the table's and the lookups' own. */
#define CSTRIPE_MAX_EXPRS      8
#define CSTRIPE_MAX_EXPR_OPS   48
#define CSTRIPE_MAX_EXPR_DEPTH 8
typedef enum cstripe_exop {
    CSTRIPE_EX_COL = 0,   /* push column `column` (NULL when the row's value is NULL) */
    CSTRIPE_EX_CONST,     /* push ival */
    CSTRIPE_EX_NULL,      /* push NULL */
    CSTRIPE_EX_ADD, CSTRIPE_EX_SUB, CSTRIPE_EX_MUL, CSTRIPE_EX_DIV, CSTRIPE_EX_MOD, CSTRIPE_EX_NEG,
    CSTRIPE_EX_LT, CSTRIPE_EX_LE, CSTRIPE_EX_GT, CSTRIPE_EX_GE, CSTRIPE_EX_EQ, CSTRIPE_EX_NE,   /* -> 0 / 1 */
    CSTRIPE_EX_AND, CSTRIPE_EX_OR, CSTRIPE_EX_NOT,      /* SQL three-valued; truth = nonzero; -> 0 / 1 / NULL */
    CSTRIPE_EX_IS_NULL,                                  /* -> 0 / 1, never NULL */
    CSTRIPE_EX_COALESCE,                                 /* (a b) -> a if a is not NULL else b */
    CSTRIPE_EX_SELECT,                                   /* (c a b) -> a if c is non-NULL and nonzero else b: CASE WHEN c THEN a ELSE b */
    CSTRIPE_EX_YEAR,                                     /* days since 1970-01-01 (this ABI's date32) -> proleptic Gregorian year */
} cstripe_exop;
typedef struct cstripe_expr_op { uint32_t op; uint32_t column; int64_t ival; } cstripe_expr_op;
typedef struct cstripe_expr    { const cstripe_expr_op *ops; uint32_t n_ops; uint32_t _pad; } cstripe_expr;

/* scan_begin_exprs: scan_begin_lookups plus expressions. With n_exprs == 0 it
 * is exactly cstripe_scan_begin_lookups (which calls it). Programs are copied.
 *  - Computed columns: expression e is column cstripe_column_count(r) + (all
 *    lookup payloads) + e, type I64. It is always projected (no cols_mask bit)
 *    and takes one of the 16 projected slots of a scan; overflow is
 *    CSTRIPE_ERR_ARG from cstripe_gpu_stage, naming the expression, and leaves
 *    the scan unstaged. Table plus derived plus computed columns must stay
 *    <= 64. cstripe_scan_column_count counts them; for such a scan the
 *    per-column arrays of cstripe_rows have that many entries.
 *  - Inputs: EX_COL names a table column of type I8/I16/I32/I64 or a
 *    lookup-derived column; every input column (and a lookup's key) is
 *    projected implicitly. F32/F64/TEXT/VARTEXT columns and other computed
 *    columns are refused at begin (SELECT nesting covers what chaining would).
 *  - Value semantics, per row, those of PG int8. Every stack entry carries a
 *    value, a NULL bit and an ERROR bit.
 *      Strict ops — ADD SUB MUL DIV MOD NEG, the six comparisons, YEAR: a NULL
 *      operand gives NULL and raises nothing (PG does not call a strict
 *      function on NULL). With all operands non-NULL: ADD / SUB / MUL / NEG
 *      beyond int64 is the error "bigint out of range"; DIV truncates toward
 *      zero, a zero divisor is "division by zero", INT64_MIN / -1 is "bigint
 *      out of range"; MOD takes the dividend's sign, a zero divisor is
 *      "division by zero", x % -1 is 0; YEAR of a value outside
 *      [-2^31, 2^31) is "year out of range". A comparison gives 0 / 1.
 *      AND / OR / NOT are Kleene over truth = nonzero: FALSE AND NULL = FALSE,
 *      TRUE OR NULL = TRUE, NOT NULL = NULL; results are 0 / 1 / NULL.
 *      IS_NULL gives 0 / 1. COALESCE (a b) is a unless a is NULL, then b.
 *      SELECT (c a b) is a when c is non-NULL and nonzero, else b.
 *    Errors are lazy, like PG's: a strict op's result is in error if an
 *    operand is or the op itself fails (a NULL result carries no error of the
 *    op itself, only its operands'); SELECT is in error if c is, otherwise it
 *    takes only the chosen branch's bit; COALESCE takes a's bit, and b's only
 *    when a is NULL; AND / OR evaluate left to right, and a clean left operand
 *    that decides the result (FALSE for AND, TRUE for OR) hides the right
 *    operand's error; NOT and IS_NULL pass their operand's bit on. So
 *    `CASE WHEN b <> 0 THEN a / b ELSE 0 END` is safe.
 *  - If the FINAL value of any row of any selected chunk group is in error,
 *    cstripe_gpu_stage returns CSTRIPE_ERR_ARG with "expression <e>: division
 *    by zero" / "bigint out of range" / "year out of range" and the scan is
 *    left unstaged.
 *  - The one deviation from PG: the stage evaluates EVERY row of the selected
 *    chunk groups, including rows the scan's predicates would reject (PG would
 *    have filtered them before ExecProject). Guard such cases with SELECT.
 *  - A computed id is accepted as the predicate column of LT..NE (a NULL
 *    operand fails the atom; column-versus-column is `computed == 1`), as the
 *    operand of COUNT_COL and every I64 aggregate kind in any operand
 *    position, as a cstripe_scan_agg_hashed / _hashed_topn key and KEY order
 *    term, as a cstripe_scan_select_topn order column, and as a wanted column
 *    of cstripe_scan_select / _select_topn. Refused with a message: IN /
 *    NOT_IN on it, cstripe_scan_agg_grouped keys, a lookup key column.
 *    cstripe_scan_next_batch and cstripe_read_row do not know it.
 *  - Key packing: the column's [lo, hi] and non-NULL count are measured by the
 *    evaluation kernel at stage (cstripe_scan_expr_range).
 *  - Errors at begin (NULL, message naming the expression and op index):
 *    n_exprs > CSTRIPE_MAX_EXPRS, n_ops 0 or above CSTRIPE_MAX_EXPR_OPS, an
 *    unknown op, stack underflow, depth above CSTRIPE_MAX_EXPR_DEPTH, a final
 *    depth other than 1, a bad or wrongly typed column.
 *  - Chunk refutation: an atom on a computed column never refutes, and the
 *    device prune kernel is skipped when one is present. A caller who wants
 *    pruning adds a redundant predicate on the base column.
 *  - Device evaluation: all at cstripe_gpu_stage, after the lookups; no query
 *    kernel knows about expressions. One launch per expression, one block per
 *    chunk group, writes the column's exists bitmap, rank table and compacted
 *    values; it then reads as an ordinary sparse I64 column in scratch. Such
 *    scans report CSTRIPE_AGG_PATH_GENERAL. A restage re-evaluates.
 *  - Out of scope: float / TEXT / VARTEXT operands or results, expressions
 *    over other expressions or over aggregates, LIKE as an expression op
 *    (LIKE / NOT LIKE are predicates on a VARTEXT table column, accepted
 *    here as by cstripe_scan_begin_ex), pruning through an expression, a dense result form, computed columns in next_batch /
 *    read_row. */
cstripe_scan *cstripe_scan_begin_exprs(cstripe_reader *r, uint64_t cols_mask,
                                       const cstripe_pred *preds, uint32_t n_preds,
                                       const cstripe_text_const *text_consts,
                                       uint32_t n_text_consts,
                                       const cstripe_value_set *sets, uint32_t n_sets,
                                       const cstripe_lookup *lookups, uint32_t n_lookups,
                                       const cstripe_expr *exprs, uint32_t n_exprs);
/* [min, max] and non-NULL count of computed column e over the selected chunk
 * groups, measured at the last stage; an all-NULL column reports
 * n_present = 0, lo = hi = 0. CSTRIPE_ERR_NOGPU on an unstaged scan,
 * CSTRIPE_ERR_ARG when e is not an expression of this scan. Any out pointer
 * may be NULL. */
int cstripe_scan_expr_range(const cstripe_scan *s, uint32_t e, int64_t *lo, int64_t *hi,
                            uint64_t *n_present);
/* device time (hipEvents, milliseconds) of the last cstripe_gpu_stage's
 * evaluation launches, all expressions together; 0 without an expression */
int cstripe_scan_last_expr_ms(const cstripe_scan *s, double *eval_ms);
void cstripe_scan_end(cstripe_scan *s);
int64_t cstripe_scan_chunk_groups_filtered(const cstripe_scan *s);

/* GPU staging: hipMalloc + HtoD copy of the selected chunks' compressed value
 * streams and exists streams for projected columns; builds device chunk
 * descriptors. Required before cstripe_scan_agg / GPU next_batch.
 * device_id < 0 => current device. */
int cstripe_gpu_stage(cstripe_scan *s, int device_id);
/* bytes staged to HBM (compressed value streams + exists bitmaps) */
uint64_t cstripe_gpu_staged_bytes(const cstripe_scan *s);

/* The sorted dictionary of a projected VARTEXT column of a staged scan:
 * *n entries in memcmp order, entry i = (*bytes)[(*offsets)[i] ..
 * (*offsets)[i+1]); rank i everywhere in this scan's results means that
 * string. The pointers are into scan-owned host memory, valid until
 * cstripe_scan_end or a restage. CSTRIPE_ERR_NOGPU on an unstaged scan,
 * CSTRIPE_ERR_ARG when col is not a projected VARTEXT column. */
int cstripe_scan_text_dict(const cstripe_scan *s, uint32_t col, uint32_t *n,
                           const uint64_t **offsets, const uint8_t **bytes);
/* device time (hipEvents, milliseconds) of the last cstripe_gpu_stage's
 * VARTEXT work, all text columns together: stream decode, header walk,
 * dictionary build (table insert + gather), rank remap. All 0 when the scan
 * projects no VARTEXT column. Any out pointer may be NULL. */
int cstripe_scan_last_text_ms(const cstripe_scan *s, double *decode_ms, double *walk_ms,
                              double *dict_ms, double *remap_ms);

/* The fused hot path: decode(LZ4) -> filter -> partial aggregate, on device.
 * Writes one partial per agg spec. Re-invocable (re-runs over staged data;
 * rescan semantics of columnar_rescan). Plain aggregate (no grouping). */
int cstripe_scan_agg(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                     cstripe_partial *partials_out);

/* GROUP BY variant (Q1 shape): group_cols = up to 2 columns of type I8.
 * partials_out sized CSTRIPE_MAX_GROUPS * n_aggs; result keys/groups in gr. */
int cstripe_scan_agg_grouped(cstripe_scan *s, const cstripe_agg_spec *aggs,
                             uint32_t n_aggs, const uint32_t *group_cols,
                             uint32_t n_group_cols, cstripe_group_result *gr,
                             cstripe_partial *partials_out);

/* Random-access read — ColumnarReadRowByRowNumber
 * (columnar_reader.c:386-441): reads the row with the given row number
 * (0-based scan-order position over the file/shard directory) into the
 * caller's per-column buffers: col_values[c] points at one value slot of
 * column c's physical width (unprojected columns may be NULL), col_nulls[c]
 * gets 0/1. Returns CSTRIPE_OK, CSTRIPE_END when no such row exists (the
 * reference returns false), or an error. Requires a scan begun WITHOUT
 * predicates — the reference's random-access path passes empty clause
 * lists the same way (:423-424). The containing chunk is device-decoded
 * and cached across consecutive calls, like the reference keeping the
 * current stripe open. */
int cstripe_read_row(cstripe_scan *s, uint64_t row_number,
                     void **col_values, uint8_t *col_nulls);

/* Batch access (parity path): returns CSTRIPE_OK with a filled batch, or
 * CSTRIPE_END when exhausted. GPU-decodes chunk by chunk and copies back;
 * residual (non-pruned-chunk) predicate filtering is NOT applied — caller
 * sees all rows of surviving chunks, as ColumnarReadNextRow does before
 * ExecQual. */
int cstripe_scan_next_batch(cstripe_scan *s, cstripe_batch *batch);
int cstripe_scan_rewind(cstripe_scan *s);

/* ---- filtered row materialisation (device-side SELECT ... WHERE) ----
 * The qual loop of ColumnarScanNext (columnar_customscan.c:1854-1913: read a
 * row, run ExecQual, return the rows that pass) with the ROWS coming out, in
 * column-major form, instead of an aggregate over them. Caller provides the
 * destinations; capacity is in rows. */
typedef struct cstripe_rows {
    uint64_t   n_rows;       /* out: rows that passed, in scan order */
    void     **col_values;   /* in: [n_cols] destinations, each >= capacity*width;
                              * NULL = column not wanted */
    uint8_t  **col_nulls;    /* in: [n_cols] or NULL; 1 = null, like cstripe_batch */
    uint64_t  *row_numbers;  /* in: capacity entries, or NULL */
} cstripe_rows;

/* cstripe_scan_select_count: number of rows cstripe_scan_select returns.
 * Runs the predicate pass on device (one pass bit per row + a prefix scan
 * of per-tile counts) and keeps both on the scan; a following
 * cstripe_scan_select reuses them. Predicates are fixed at scan_begin, so
 * only cstripe_scan_end / a restage drops that cache.
 *
 * cstripe_scan_select:
 *  - Filter: a row passes iff the scan's CNF predicate set is true,
 *    evaluated exactly as cstripe_scan_agg evaluates it — OR groups, a NULL
 *    operand fails its atom, PG float ordering (NaN greatest, equal to
 *    itself), TEXT compares whole slots; zero predicates select every row.
 *    Chunk groups removed by min/max pruning contribute nothing.
 *  - Order: scan order (ascending row number), deterministic, identical on
 *    every call.
 *  - Values: written at the column's physical width in the ABI's raw
 *    representation (TEXT = the 4-byte slot); NULL slots are zero-filled
 *    with col_nulls[c][i] = 1. A wanted column must be projected (in
 *    cols_mask or a predicate column), else CSTRIPE_ERR_ARG.
 *  - Row numbers: the reference's rowNumber out-parameter
 *    (ColumnarReadNextRow, columnar_reader.c:322-361) — the 0-based
 *    table-wide row position cstripe_read_row accepts on a predicate-free
 *    scan of the same reader: cumulative rows over ALL chunk groups in
 *    directory order, so a surviving chunk's base counts the pruned chunks
 *    before it, and positions continue across shard files.
 *  - Capacity: capacity < n_rows returns CSTRIPE_ERR_ARG (the message names
 *    both numbers) and writes nothing.
 *  - Destinations: dst_on_device != 0 — every destination pointer is device
 *    memory on the scan's device and results never touch the host (they can
 *    feed cstripe_write_rows_device directly). Otherwise destinations are
 *    host memory: the library compacts into a device buffer it owns, sized
 *    by the count, and issues one DtoH copy per wanted stream.
 *  - Errors: both need a staged scan (CSTRIPE_ERR_NOGPU otherwise); a device
 *    decode error flag surfaces as CSTRIPE_ERR_FORMAT.
 *  - Both are re-invocable and may be interleaved with scan_agg,
 *    scan_agg_grouped, next_batch and read_row on the same scan without
 *    changing any of their results. Decode kernels re-run per call, like
 *    cstripe_scan_agg. cstripe_scan_last_kernel_ms /
 *    cstripe_scan_last_decode_kernel_ms then report the last select (or
 *    select_count) call.
 *  - Zero selected chunk groups or zero passing rows: CSTRIPE_OK, n_rows = 0. */
int cstripe_scan_select_count(cstripe_scan *s, uint64_t *n_rows);
int cstripe_scan_select(cstripe_scan *s, cstripe_rows *out,
                        uint64_t capacity, int dst_on_device);
/* per-kernel device time of the last select / select_count call,
 * milliseconds; a pass that was served from the scan's cache reads 0.
 * Any out pointer may be NULL. */
int cstripe_scan_last_select_ms(const cstripe_scan *s, double *mask_ms,
                                double *offsets_ms, double *emit_ms);

/* ---- ORDER BY ... LIMIT over the scan (device top-N) ----
 * What the reference pushes to every worker: WorkerLimitCount and
 * WorkerSortClauseList (multi_logical_optimizer.c:5038-5212) hand each shard
 * ORDER BY ... LIMIT limit+offset, and the coordinator re-sorts the few rows
 * it gets back. The device finds the limit-th smallest key without sorting
 * (an 8-bit-per-round radix select) and compacts exactly those rows. */
#define CSTRIPE_MAX_ORDER_COLS    4
#define CSTRIPE_MAX_TOPN          (1u << 20)
#define CSTRIPE_ORDER_DESC        1u
#define CSTRIPE_ORDER_NULLS_FIRST 2u     /* absent = NULLS LAST */
typedef struct cstripe_order_key { uint32_t column; uint32_t flags; } cstripe_order_key;

/* cstripe_scan_select_topn:
 *  - Rows: those that pass the scan's CNF, evaluated exactly as
 *    cstripe_scan_select evaluates it; chunk groups removed by min/max
 *    pruning contribute nothing. out->n_rows = min(limit, passing rows).
 *    Every destination in `out` holds `limit` entries. Values, NULL
 *    zero-fill, null bytes, row numbers and device / host destinations
 *    follow cstripe_scan_select; a wanted column must be projected.
 *  - Order: lexicographic over order[0..n_order), each column ascending, or
 *    descending with CSTRIPE_ORDER_DESC. NULLs sort after every value of the
 *    column, or before it with CSTRIPE_ORDER_NULLS_FIRST — the flag is taken
 *    literally (PG's defaults, ASC -> LAST and DESC -> FIRST, are the
 *    caller's job). Integers compare signed; F32/F64 compare in PG order
 *    (NaN greatest and equal to itself, -0.0 = +0.0); VARTEXT compares by
 *    dictionary rank, which is memcmp order. Rows equal on the whole key
 *    tuple come out in ascending row number, so the result is fully
 *    determined and identical on every call.
 *  - Key types: I8/I16/I32/I64/F32/F64/VARTEXT. A TEXT order column is
 *    CSTRIPE_ERR_ARG: its row-level order in this ABI is whole-slot, not
 *    collation, and the message says so.
 *  - Key packing (the supported domain): as in cstripe_scan_agg_hashed the
 *    key tuple is ONE 64-bit word. Per column [lo, hi] comes from the skip
 *    nodes (min/max) of the scan's SELECTED chunk groups; a selected chunk
 *    with present values and no min/max widens the column to its type's full
 *    range; VARTEXT uses [0, n_dict - 1]. Floats go through an
 *    order-preserving map `ord` of the f64 bit pattern (F32 widened exactly;
 *    every NaN maps to ord(+inf) + 1, -0.0 to +0.0; the skip nodes' float
 *    min/max are already in PG order). A column needs
 *    bitlen(ord(hi) - ord(lo) + 1) bits: the value offsets plus one NULL
 *    code at either end. Column 0 is most significant. A total above 64 bits
 *    is CSTRIPE_ERR_ARG, the message naming each column's bits. A value
 *    outside [lo, hi] (a file whose skip nodes lie) raises a device flag and
 *    returns CSTRIPE_ERR_FORMAT, never a wrong row.
 *  - Errors: an unstaged scan returns CSTRIPE_ERR_NOGPU, checked first,
 *    before any argument. CSTRIPE_ERR_ARG: limit 0 or above
 *    CSTRIPE_MAX_TOPN, n_order 0 or above CSTRIPE_MAX_ORDER_COLS, an order
 *    column out of range or not projected, a repeated order column. Zero
 *    selected chunk groups or zero passing rows: CSTRIPE_OK, n_rows = 0.
 *  - Memory: the device key array costs 8 bytes per PASSING row (not per
 *    returned row), plus two mask bits per scanned row; both hang off the
 *    scan, grow on demand and are freed by cstripe_scan_end.
 *  - Re-invocable, and may be interleaved with every other scan call
 *    without changing any of their results: it uses (and, when absent,
 *    fills) the pass mask, tile counts and bases cstripe_scan_select caches,
 *    and never writes into them — its refined mask and bases live in
 *    buffers of their own. cstripe_scan_last_kernel_ms /
 *    cstripe_scan_last_decode_kernel_ms then report this call;
 *    cstripe_scan_last_topn_ms splits out the key build, the selection (all
 *    histogram, pick and refine launches; 0 when passing rows <= limit) and
 *    the final emit plus permute. Any out pointer may be NULL. */
int cstripe_scan_select_topn(cstripe_scan *s, const cstripe_order_key *order,
                             uint32_t n_order, uint64_t limit,
                             cstripe_rows *out, int dst_on_device);
int cstripe_scan_last_topn_ms(const cstripe_scan *s, double *key_ms,
                              double *select_ms, double *emit_ms);

/* ---- hashed GROUP BY (device hash aggregate over integer keys) ----
 * The worker side of the reference's general grouped plan: HashAggregate
 * over ColumnarScan, one partial row per group, then a per-group coordinator
 * merge (multi_explain.out:80-82, multi_logical_optimizer.c:1807-1885,
 * aggregate_utils.c:820-1021). Unlike cstripe_scan_agg_grouped (Q1 shape,
 * <= 64 groups of char(1) keys) the group count is bounded only by the
 * caller's capacity. Caller provides every destination; capacity is in
 * groups. */
#define CSTRIPE_MAX_HASH_KEY_COLS 4
#define CSTRIPE_MAX_HASH_GROUPS   (1u << 24)

typedef struct cstripe_hgroups {
    uint64_t         n_groups;                               /* out */
    int64_t         *keys[CSTRIPE_MAX_HASH_KEY_COLS];        /* in: capacity entries each (first n_key_cols used) */
    uint8_t         *key_nulls[CSTRIPE_MAX_HASH_KEY_COLS];   /* in: capacity bytes each; 1 = NULL key */
    cstripe_partial *partials;                               /* in: capacity * n_aggs, [g*n_aggs + a] */
} cstripe_hgroups;

/* cstripe_scan_agg_hashed:
 *  - Keys: 1..CSTRIPE_MAX_HASH_KEY_COLS columns of type I8/I16/I32/I64/TEXT.
 *    F32/F64 keys, zero key columns (that is cstripe_scan_agg), more than
 *    4, or a key column that is not projected return CSTRIPE_ERR_ARG. A key
 *    value comes back sign-extended in keys[k][g]; TEXT returns the whole
 *    4-byte slot zero-extended (TEXT groups by slot here, not by first
 *    payload byte — for char(1) the two are the same). NULL keys form their
 *    own group, like the reference's HashAggregate (grouping treats NULLs
 *    as equal): key_nulls[k][g] = 1, keys[k][g] = 0. A VARTEXT key column
 *    packs its dictionary rank over [0, n_dict - 1] (not the skip-node
 *    range) and returns the rank; cstripe_scan_text_dict decodes it.
 *  - Filter, aggregates, NULL operands, PG NaN order, is_null, COUNT never
 *    null: exactly as cstripe_scan_agg_grouped — the same 11 agg kinds, the
 *    same accumulator-to-partial conversion, int128 sums exact. Chunk groups
 *    removed by min/max pruning contribute nothing.
 *  - Order: each distinct key tuple appears exactly once; groups are sorted
 *    ascending by key tuple, column 0 most significant, signed compare, per
 *    column NULL last (PG's ASC defaults to NULLS LAST). Identical on every
 *    call.
 *  - Capacity: 1..CSTRIPE_MAX_HASH_GROUPS, else CSTRIPE_ERR_ARG. The device
 *    table has slots = max(2, next_pow2(2*capacity)). More groups than
 *    capacity returns CSTRIPE_ERR_ARG and writes nothing: the message names
 *    the exact group count and the capacity when the table did not fill,
 *    and says "more than <slots> groups" when it did.
 *  - Key packing (the supported domain): the device key is ONE 64-bit word.
 *    Per key column the library takes [lo, hi] from the skip nodes
 *    (min/max) of the scan's SELECTED chunk groups; a selected chunk with
 *    present values and no min/max widens that column to its type's full
 *    range; TEXT always uses the slot as u32, 0..2^32-1 (its skip-node
 *    min/max are order keys, not slots). A column's code is 0 for NULL,
 *    else 1 + (v - lo), in bitlen(hi - lo + 1) bits. The bits of all key
 *    columns must total <= 63; wider key tuples return CSTRIPE_ERR_ARG (the
 *    message names each column's bits) — not pushdownable through this ABI,
 *    like an over-wide CNF. One extension past whole-slot TEXT packing:
 *    when the total exceeds 63 bits and TEXT key columns are among them
 *    (two char(1) flags are already 66), those columns pack by their
 *    C-collation order key instead, whose [min, max] the skip nodes do
 *    record; keys still come back as slots, sorted by slot value. That
 *    form needs canonical short-varlena slots (header = payload length,
 *    zero padding); the kernel checks every slot and any other slot fails
 *    the call with CSTRIPE_ERR_ARG. A value outside [lo, hi] (a file whose skip
 *    nodes lie) surfaces as CSTRIPE_ERR_FORMAT, never as a wrong group.
 *  - Needs a staged scan (CSTRIPE_ERR_NOGPU otherwise; checked first). Zero
 *    selected chunk groups or zero passing rows: CSTRIPE_OK, n_groups = 0.
 *  - Re-invocable, and may be interleaved with scan_agg, scan_agg_grouped,
 *    scan_select, next_batch and read_row on the same scan without changing
 *    any of their results. cstripe_scan_last_kernel_ms /
 *    cstripe_scan_last_decode_kernel_ms then report the last hashed call;
 *    cstripe_scan_last_hash_ms splits the device time per kernel (table
 *    init, scan + hash aggregate, compaction); any out pointer may be NULL.
 *  - CSTRIPE_HASH_LDS_SLOTS (environment, read per call) overrides the
 *    per-block LDS table's slot count: 0 = no LDS table, a small power of
 *    two forces overflow into the global table. Results do not depend on
 *    it. */
int cstripe_scan_agg_hashed(cstripe_scan *s, const cstripe_agg_spec *aggs, uint32_t n_aggs,
                            const uint32_t *key_cols, uint32_t n_key_cols,
                            uint64_t capacity, cstripe_hgroups *out);
int cstripe_scan_last_hash_ms(const cstripe_scan *s, double *init_ms, double *scan_ms, double *compact_ms);

/* ---- GROUP BY ... [HAVING] ORDER BY ... LIMIT (device top-N over groups) ----
 * The last step of the reference's pushed-down grouped plan. WorkerLimitCount
 * (multi_logical_optimizer.c:5039-5140) hands each shard the exact LIMIT
 * limit+offset with the ORDER BY when the GROUP BY holds the partition column
 * (groupedByDisjointPartitionColumn, :5081-5085 — every group lives on one
 * shard), and an approximate row count when the ORDER BY names a commutative
 * aggregate (:5094-5111); WorkerSortClauseList (:5163-5212) supplies the
 * order, and HAVING goes to the worker in the same disjoint case
 * (ProcessHavingClauseForWorkerQuery, :2650-2682). Here the group table of
 * cstripe_scan_agg_hashed stays in HBM, a set of kernels filters, ranks and
 * selects over it, and only `limit` groups are copied back. */
#define CSTRIPE_MAX_GROUP_ORDER 4
#define CSTRIPE_MAX_HAVING      4
#define CSTRIPE_GORDER_AGG 0u      /* index = position in aggs[]     */
#define CSTRIPE_GORDER_KEY 1u      /* index = position in key_cols[] */
typedef struct cstripe_group_order {
    uint32_t kind;     /* CSTRIPE_GORDER_* */
    uint32_t index;
    uint32_t flags;    /* CSTRIPE_ORDER_DESC | CSTRIPE_ORDER_NULLS_FIRST, taken
                        * literally as in cstripe_scan_select_topn */
    uint32_t _pad;
} cstripe_group_order;
typedef struct cstripe_having {
    uint32_t agg;      /* position in aggs[] */
    uint32_t op;       /* CSTRIPE_PRED_LT .. CSTRIPE_PRED_NE; atoms are ANDed */
    int64_t  ival;     /* constant for COUNT and integer kinds */
    double   fval;     /* constant for f64 kinds */
} cstripe_having;

/* cstripe_scan_agg_hashed_topn:
 *  - Groups, aggregates, filter, NULL keys: exactly cstripe_scan_agg_hashed —
 *    the same key types, packing, 63-bit rule, `capacity` / slots and error
 *    messages (they keep the scan_agg_hashed prefix: one front half serves
 *    both calls); CSTRIPE_HASH_LDS_SLOTS is honoured; lookup-derived and
 *    VARTEXT key columns are accepted. `capacity` bounds the number of groups
 *    BEFORE HAVING. Every destination in `out` holds `limit` entries.
 *  - HAVING: a group survives iff every atom is true on the aggregate's final
 *    value. COUNT kinds compare the count with ival; integer kinds compare
 *    the full int128 with ival, exactly (a sum beyond 64 bits still compares
 *    correctly); f64 kinds compare with fval in PG float order (NaN greatest
 *    and equal to itself, -0.0 = +0.0). A NULL aggregate (no contributing
 *    row) fails its atom. n_having == 0 keeps every group.
 *  - Order: lexicographic over order[0..n_order). An AGG term orders by the
 *    aggregate's value — signed for COUNT and integer kinds, PG float order
 *    for f64 kinds; a NULL aggregate sorts after every value, or before with
 *    CSTRIPE_ORDER_NULLS_FIRST. A KEY term orders by that key column's value
 *    as cstripe_scan_select_topn orders the column (VARTEXT by rank, a NULL
 *    key last or first by the flag). Groups equal on every term come out
 *    ascending by key tuple exactly as cstripe_scan_agg_hashed sorts them
 *    (column 0 most significant, signed, NULL last, TEXT by slot value). The
 *    result is a total order, independent of the table's slot order and
 *    identical on every call; n_order == 0 is legal and means "the first
 *    `limit` surviving groups in key order". One stated exception: a SUM_F64
 *    term is only as reproducible as the atomic f64 sum itself.
 *  - Result: out->n_groups = min(limit, surviving groups), in the requested
 *    order; keys, key_nulls and partials converted exactly as
 *    cstripe_scan_agg_hashed converts them.
 *  - Supported domain: the ORDER terms pack into ONE 64-bit order word, term
 *    0 most significant. An AGG term's [lo, hi] is measured on the device
 *    over the surviving non-NULL groups and needs bitlen(hi - lo + 1) bits —
 *    the value offsets plus one NULL code at either end; a KEY term uses the
 *    range the key packing derived. (An f64 term is measured in order codes
 *    of the bit pattern: values of one sign and similar magnitude take few
 *    bits, values of both signs take all 64, leaving room for no other
 *    term.) More than 64 bits is CSTRIPE_ERR_ARG, the
 *    message naming each term's bits. An integer AGG order term whose value
 *    in some surviving group does not fit int64 is CSTRIPE_ERR_ARG naming the
 *    aggregate (HAVING has no such limit). The tie word is the key tuple
 *    re-packed in output order, at most 63 bits.
 *  - Errors: an unstaged scan returns CSTRIPE_ERR_NOGPU, checked first.
 *    CSTRIPE_ERR_ARG: limit 0 or above CSTRIPE_MAX_TOPN; n_order above
 *    CSTRIPE_MAX_GROUP_ORDER or n_having above CSTRIPE_MAX_HAVING; a bad
 *    kind, index, op or flags; a repeated order term; a TEXT key column named
 *    as a KEY order term (the message of cstripe_scan_select_topn); a key
 *    tuple that only packs through the TEXT order-key fallback (use
 *    cstripe_scan_agg_hashed); everything cstripe_scan_agg_hashed rejects.
 *    Zero selected chunk groups, zero passing rows or zero surviving groups:
 *    CSTRIPE_OK, n_groups = 0.
 *  - Device work after the shared front half (table init, scan + hash
 *    aggregate, compaction): a range / HAVING kernel (kept indices, per-term
 *    min / max, the out-of-int64 flag; its small state block is the one
 *    copy-back before the selection), a key kernel (order word + tie word per
 *    kept group), the 8-bit radix select of cstripe_scan_select_topn over the
 *    order word and then over the tie word among the groups on the threshold
 *    (skipped when kept <= limit), and a gather of the selected groups. One
 *    DtoH copy of limit * (24 + 32 * n_aggs) bytes follows; the host sorts
 *    those by (order word, tie word).
 *  - Re-invocable, and may be interleaved with every other scan call without
 *    changing any of their results: its buffers are its own or the ones
 *    cstripe_scan_agg_hashed re-initialises per call.
 *    cstripe_scan_last_hash_ms reports the front half of this call;
 *    cstripe_scan_last_group_topn the groups before and after HAVING and the
 *    device time of the range / HAVING kernel, the key build plus selection,
 *    and the gather (all 0 when no group was found). Any out pointer may be
 *    NULL. */
int cstripe_scan_agg_hashed_topn(cstripe_scan *s,
        const cstripe_agg_spec *aggs, uint32_t n_aggs,
        const uint32_t *key_cols, uint32_t n_key_cols, uint64_t capacity,
        const cstripe_having *having, uint32_t n_having,
        const cstripe_group_order *order, uint32_t n_order,
        uint64_t limit, cstripe_hgroups *out);
int cstripe_scan_last_group_topn(const cstripe_scan *s, uint64_t *n_groups, uint64_t *n_kept,
        double *range_ms, double *select_ms, double *emit_ms);

/* 1 when the last cstripe_scan_agg ran the fused decode+filter+aggregate
 * kernel (no scratch round trip), 0 for the two-kernel path */
int cstripe_scan_last_fused(const cstripe_scan *s);

/* which kernel body the last cstripe_scan_agg ran */
#define CSTRIPE_AGG_PATH_NONE       0   /* no call yet, or an empty selection */
#define CSTRIPE_AGG_PATH_FUSED      1   /* fused decode+filter+aggregate */
#define CSTRIPE_AGG_PATH_GENERAL    2   /* per-row kernel (NULLs present) */
#define CSTRIPE_AGG_PATH_DENSE      3   /* dense, R-row windows per column */
#define CSTRIPE_AGG_PATH_DENSE_OV   4   /* dense, overlapped column loads */
int cstripe_scan_last_agg_path(const cstripe_scan *s);

/* per-call timing of the last cstripe_scan_agg: kernel time (hipEvents, on the
 * scan's stream) and wall time inside the call, milliseconds. */
double cstripe_scan_last_kernel_ms(const cstripe_scan *s);
double cstripe_scan_last_decode_kernel_ms(const cstripe_scan *s);
double cstripe_scan_last_agg_kernel_ms(const cstripe_scan *s);

/* =================== combine surface =================== */
/* Merge per-shard/per-GPU partials: out = combine(parts[0..n)). Reproduces
 * coord_combine_agg semantics: strict combine over non-null partials
 * (aggregate_utils.c:976-1000); COUNT kinds get NULL->0 (COALESCE,
 * multi_logical_optimizer.c:1831-1885), so a COUNT out is never null. */
int cagg_combine(const cstripe_agg_spec *aggs, uint32_t n_aggs,
                 const cstripe_partial *parts, uint32_t n_parts,
                 cstripe_partial *out);

/* The coordinator merge per group (host C, no GPU): the union of the key
 * tuples of all parts; for each key, cagg_combine over the entries that hold
 * it. Inputs may be in any order and a part may hold a key more than once
 * (those merge too); NULL keys compare equal. Output is sorted like
 * cstripe_scan_agg_hashed's. More than `capacity` result groups returns
 * CSTRIPE_ERR_ARG with the needed count in out->n_groups and writes nothing
 * else. VARTEXT keys are per-scan dictionary ranks: parts from different
 * scans do not share a coding, so merging them here is out of scope. */
int cagg_combine_groups(const cstripe_agg_spec *aggs, uint32_t n_aggs, uint32_t n_key_cols,
                        const cstripe_hgroups *parts, uint32_t n_parts,
                        cstripe_hgroups *out, uint64_t capacity);

/* =================== RCCL combine (device collective) ===================
 * The north star replaces the coordinator merge with a collective over
 * xGMI. The data-path hop is ncclAllGather of each rank's partial block
 * (RCCL over xGMI), followed by the same strict cagg_combine merge locally
 * on every rank: int128 carries cannot ride a sum collective, and gathering
 * is byte-faithful to the coordinator receiving one partial row per shard
 * (aggregate_utils.c:820-1021; adaptive_executor.c:775-882). Host code stays
 * C; the launcher only has to distribute the 128-byte unique id (the same
 * bootstrap contract as ncclCommInitRank). */
typedef struct cagg_comm cagg_comm;
#define CAGG_UNIQUE_ID_BYTES 128

int cagg_comm_unique_id(uint8_t id[CAGG_UNIQUE_ID_BYTES]);   /* rank 0 makes */
int cagg_comm_init(cagg_comm **out, int n_ranks, int rank,
                   const uint8_t id[CAGG_UNIQUE_ID_BYTES], int device);
void cagg_comm_destroy(cagg_comm *c);
int cagg_comm_rank(const cagg_comm *c);
int cagg_comm_size(const cagg_comm *c);

/* all-gather equal-size byte blocks from every rank (device-staged
 * internally; dst holds n_ranks * bytes, rank-major) */
int cagg_allgather(cagg_comm *c, const void *src, uint64_t bytes, void *dst);

/* the combine surface over RCCL: gather every rank's partial block, then
 * cagg_combine locally; every rank returns the final merged row */
int cagg_combine_rccl(cagg_comm *c, const cstripe_agg_spec *aggs,
                      uint32_t n_aggs, const cstripe_partial *local,
                      cstripe_partial *out);

/* =================== misc =================== */
const char *cstripe_errmsg(void);
int cstripe_gpu_available(void);     /* 1 if a HIP device is visible */
uint32_t cstripe_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSTRIPE_H */

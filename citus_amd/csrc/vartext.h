/*
 * vartext.h — the varlena header walk of a CSTRIPE_VARTEXT value stream,
 * shared by the writer's self-check, cstripe_vartext_validate (host) and the
 * device walk kernel (cstripe_gpu.hip).
 *
 * The stream is what the reference writes for a text column
 * (SerializeSingleDatum, columnar_writer.c:555-585, typalign 'i') and walks
 * back with fetch_att / att_addlength_datum / att_align_nominal
 * (DeserializeDatumArray, columnar_reader.c:1542-1572): present values only,
 * each datum
 *     total <= 127 : 1-byte header (total << 1) | 1, payload
 *     otherwise    : 4-byte little-endian header total << 2, payload
 * (total counts the header bytes) and then zero padding to the next 4-byte
 * boundary, so every datum starts 4-aligned.
 */
#ifndef CSTRIPE_VARTEXT_H
#define CSTRIPE_VARTEXT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CSVT_HD __host__ __device__
#else
#define CSVT_HD
#endif

#define CSVT_MAX_LEN 65535u   /* == CSTRIPE_VARTEXT_MAX_LEN */

/* One step of the walk. `hdr` points at a datum's first byte and `avail` is
 * the number of stream bytes from there to the stream's end (only hdr[0] is
 * read when avail < 4). On success returns 0 and sets the payload's offset
 * from `hdr`, its length, and the distance to the next datum (total rounded
 * up to 4; it may reach past `avail` by the final datum's padding only).
 * Nonzero: the datum is malformed or overruns the stream —
 *   1 header form this format never writes (compressed / external varlena)
 *   2 total smaller than its own header
 *   3 datum overruns the stream
 *   4 payload longer than CSVT_MAX_LEN */
static inline CSVT_HD int csvt_step(const uint8_t *hdr, uint64_t avail,
                                    uint32_t *pay_off, uint32_t *pay_len,
                                    uint32_t *advance)
{
    if (avail == 0) return 3;
    const uint32_t b0 = hdr[0];
    uint32_t hlen, total;
    if (b0 & 1u) {
        hlen = 1;
        total = b0 >> 1;
    } else if ((b0 & 3u) == 0) {
        if (avail < 4) return 3;
        hlen = 4;
        total = (b0 | ((uint32_t)hdr[1] << 8) | ((uint32_t)hdr[2] << 16) |
                 ((uint32_t)hdr[3] << 24)) >> 2;
    } else {
        return 1;
    }
    if (total < hlen) return 2;
    if (total > avail) return 3;
    if (total - hlen > CSVT_MAX_LEN) return 4;
    *pay_off = hlen;
    *pay_len = total - hlen;
    *advance = (total + 3u) & ~3u;
    return 0;
}

/* 0 when exactly n_values datums tile stream[0..len): every datum fits, and
 * the walk reaches the end (the last datum's padding may be cut) after
 * n_values steps, not sooner and not later */
static inline CSVT_HD int csvt_validate(const uint8_t *stream, uint64_t len,
                                        uint32_t n_values)
{
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n_values; i++) {
        if (pos >= len) return 5;                 /* fewer datums than claimed */
        uint32_t po, pl, adv;
        const int rc = csvt_step(stream + pos, len - pos, &po, &pl, &adv);
        if (rc) return rc;
        pos += adv;
    }
    return pos >= len ? 0 : 6;                    /* more datums than claimed */
}

/* Skip-node order key of a value: its first 7 payload bytes big-endian in
 * bits 55..0, zero-padded — a non-negative int64, monotone under memcmp
 * order (a <= b implies key(a) <= key(b)) and not injective: values sharing
 * a 7-byte prefix share a key, and so do "ab" and "ab\0..." (text holds no
 * NUL, so only the former matters). */
static inline CSVT_HD int64_t csvt_prefix_key(const uint8_t *p, uint32_t len)
{
    uint64_t k = 0;
    for (uint32_t i = 0; i < 7; i++)
        k = (k << 8) | (i < len ? p[i] : 0u);
    return (int64_t)k;
}

#endif /* CSTRIPE_VARTEXT_H */

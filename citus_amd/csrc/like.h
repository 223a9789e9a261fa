/*
 * like.h — the LIKE pattern matcher of CSTRIPE_PRED_LIKE / NOT_LIKE, shared
 * by cstripe_like_match and scan_begin's pattern check (host) and the device
 * match kernel (vt_like_kernel, cstripe_gpu.hip).
 *
 * The language is PG LIKE with the default escape, "C" collation, UTF-8
 * (MatchText, like_match.c): '%' any run of characters, '_' one character,
 * '\x' the byte x, any other byte itself; a character is one byte plus the
 * continuation bytes ((b & 0xC0) == 0x80) after it (NextChar); anchored at
 * both ends.
 *
 * One loop, no recursion, no stack memory: two cursors, the pattern position
 * after the last '%' and the text position that '%' currently stands at. On
 * a mismatch the '%' swallows one more character and both cursors restart
 * there. Every restart moves the text restart point forward, and between
 * restarts the pattern cursor only advances, so a match takes at most
 * (vlen + 1) * (plen + 1) steps. Restarting only the last '%' is sufficient:
 * an earlier '%' that swallowed more would leave the later one a suffix of
 * the text it already searched.
 *
 * Exact for valid UTF-8 (ASCII included). On bytes that are not valid UTF-8
 * the verdict is unspecified — the restart point skips continuation bytes,
 * which PG's recursive matcher does not always do — but it is deterministic,
 * terminates within the bound above and reads only pat[0..plen) and
 * val[0..vlen).
 */
#ifndef CSTRIPE_LIKE_H
#define CSTRIPE_LIKE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CSLK_HD __host__ __device__
#else
#define CSLK_HD
#endif

#define CSLK_MAX_PATTERN 256u   /* == CSTRIPE_LIKE_MAX_PATTERN */

/* pattern check of scan_begin and cstripe_like_match:
 *   0 fine
 *   1 longer than CSLK_MAX_PATTERN
 *   2 ends in an unescaped backslash
 *   3 not valid UTF-8 (overlong forms, surrogates and code points above
 *     U+10FFFF included) */
static inline CSLK_HD int cslk_check_pattern(const uint8_t *pat, uint32_t plen)
{
    if (plen > CSLK_MAX_PATTERN) return 1;
    uint32_t i = 0;
    while (i < plen) {
        const uint32_t b = pat[i];
        uint32_t n, lo = 0x80, hi = 0xBF;
        if (b < 0x80) { i++; continue; }
        if (b >= 0xC2 && b <= 0xDF) n = 1;
        else if (b >= 0xE0 && b <= 0xEF) {
            n = 2;
            if (b == 0xE0) lo = 0xA0;
            if (b == 0xED) hi = 0x9F;
        } else if (b >= 0xF0 && b <= 0xF4) {
            n = 3;
            if (b == 0xF0) lo = 0x90;
            if (b == 0xF4) hi = 0x8F;
        } else return 3;
        if (i + n >= plen) return 3;
        if (pat[i + 1] < lo || pat[i + 1] > hi) return 3;
        for (uint32_t k = 2; k <= n; k++)
            if ((pat[i + k] & 0xC0u) != 0x80u) return 3;
        i += n + 1;
    }
    /* a backslash escapes the byte after it: walk the pairs */
    for (i = 0; i < plen; i++)
        if (pat[i] == '\\') {
            if (i + 1 == plen) return 2;
            i++;
        }
    return 0;
}

/* 1 when val[0..vlen) matches pat[0..plen), else 0. The pattern has passed
 * cslk_check_pattern (a trailing backslash, which it refuses, would match
 * nothing here). */
static inline CSLK_HD int cslk_match(const uint8_t *pat, uint32_t plen,
                                     const uint8_t *val, uint32_t vlen)
{
    uint32_t p = 0, t = 0;
    uint32_t star_p = 0, star_t = 0;
    bool star = false;
    for (;;) {
        if (p < plen && pat[p] == '%') {
            star = true;
            star_p = ++p;
            star_t = t;
            continue;
        }
        if (t == vlen) {
            /* text used up: a match iff the pattern is too (a '%' here was
             * taken above); no longer restart point can help */
            return p == plen ? 1 : 0;
        }
        bool ok = false;
        if (p < plen) {
            if (pat[p] == '_') {
                p++;
                t++;
                while (t < vlen && (val[t] & 0xC0u) == 0x80u) t++;
                ok = true;
            } else {
                uint32_t q = p;
                if (pat[q] == '\\') q++;
                if (q < plen && pat[q] == val[t]) {
                    p = q + 1;
                    t++;
                    ok = true;
                }
            }
        }
        if (ok) continue;
        if (!star) return 0;
        /* the last '%' takes one more character */
        star_t++;
        while (star_t < vlen && (val[star_t] & 0xC0u) == 0x80u) star_t++;
        p = star_p;
        t = star_t;
    }
}

/* The literal bytes before the first unescaped '%' or '_', escapes
 * resolved, at most 7 of them (what a prefix key holds) into pre[0..7);
 * returns how many. Zero: the pattern bounds no prefix. */
static inline CSLK_HD uint32_t cslk_literal_prefix(const uint8_t *pat, uint32_t plen,
                                                   uint8_t *pre)
{
    uint32_t n = 0;
    for (uint32_t i = 0; i < plen && n < 7; i++) {
        uint8_t b = pat[i];
        if (b == '%' || b == '_') break;
        if (b == '\\') {
            if (++i == plen) break;
            b = pat[i];
        }
        pre[n++] = b;
    }
    return n;
}

#endif /* CSTRIPE_LIKE_H */

// One line of k-mer text (include/brx.h "k-mer text", br_amd/kmertext.py states it in numpy), for host and device: what a
// lane of brx_kmertext.hip's kernels does with its entry or its line.
#pragma once
#include "brx_kmer.hpp"

namespace brx {

// causes of a malformed line, in the order a line is read (kmertext.py CAUSES)
enum : uint32_t { TEXT_OK = 0, TEXT_BASE = 1, TEXT_SHORT = 2, TEXT_LONG = 3, TEXT_NOCOUNT = 4, TEXT_DIGIT = 5, TEXT_ZERO = 6 };

constexpr uint32_t TEXT_MAX_LINE = 36; // 31 letters, TAB, three digits, '\n'

BRX_HD uint32_t text_line_len(int k, uint32_t count) { return (uint32_t)k + 3u + (count >= 10u ? 1u : 0u) + (count >= 100u ? 1u : 0u); }

// A C T G = 0 1 2 3 -> A C G T = 0 1 2 3 in every 2-bit group: the order of the letters
BRX_HD uint64_t text_ascii_order(uint64_t kmer) { return kmer ^ ((kmer >> 1) & 0x5555555555555555ull); }

// the k-mer printed for key x: its canonical k-mer, or (lex) the alphabetically smaller of that and its reverse complement
BRX_HD uint64_t text_kmer_of_key(uint64_t key, int k, bool lex)
{
    const uint64_t c = (key << 1) | (uint64_t)(popc64(key) & 1);
    if (!lex)
        return c;
    const uint64_t r = revcomp(c, k);
    return text_ascii_order(r) < text_ascii_order(c) ? r : c;
}

// the line of (key, count) into out[0 .. text_line_len)
BRX_HD uint32_t text_format_line(int k, uint64_t key, uint32_t count, bool lex, uint8_t *out)
{
    const uint64_t kmer = text_kmer_of_key(key, k, lex);
    uint32_t at = 0;
    for (int i = k - 1; i >= 0; i--)
        out[at++] = bit2nuc(kmer >> (2 * i));
    out[at++] = (uint8_t)'\t';
    if (count >= 100u)
        out[at++] = (uint8_t)('0' + count / 100u);
    if (count >= 10u)
        out[at++] = (uint8_t)('0' + (count / 10u) % 10u);
    out[at++] = (uint8_t)('0' + count % 10u);
    out[at++] = (uint8_t)'\n';
    return at;
}

// a line without its '\n': one '\r' at its end is dropped; what is left may be empty
BRX_HD uint64_t text_trim(const uint8_t *p, uint64_t len) { return len && p[len - 1] == (uint8_t)'\r' ? len - 1 : len; }

// The non-empty line p[0 .. len): exactly k bases of either case, one or more of TAB / space, one or more digits, nothing
// else.  TEXT_OK: *key = canonical(k-mer) >> 1, *count = min(255, value) >= 1.  Otherwise the cause, with *col = the column
// (from 1) of the offending byte for TEXT_BASE and TEXT_DIGIT, the number of bases for TEXT_SHORT and TEXT_LONG, else 0.
BRX_HD uint32_t text_parse_line(const uint8_t *p, uint64_t len, int k, uint64_t *key, uint32_t *count, uint64_t *col)
{
    uint64_t i = 0, kmer = 0;
    *col = 0;
    for (; i < len && p[i] != (uint8_t)'\t' && p[i] != (uint8_t)' '; i++) {
        const uint8_t u = p[i] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') {
            *col = i + 1;
            return TEXT_BASE;
        }
        if (i < (uint64_t)k)
            kmer = (kmer << 2) | nuc2bit(p[i]);
    }
    if (i != (uint64_t)k) {
        *col = i;
        return i < (uint64_t)k ? TEXT_SHORT : TEXT_LONG;
    }
    while (i < len && (p[i] == (uint8_t)'\t' || p[i] == (uint8_t)' '))
        i++;
    if (i == len)
        return TEXT_NOCOUNT;
    uint32_t v = 0;
    for (; i < len; i++) {
        const uint32_t d = (uint32_t)p[i] - (uint32_t)'0';
        if (d > 9u) {
            *col = i + 1;
            return TEXT_DIGIT;
        }
        v = v * 10u + d;
        v = v > 255u ? 255u : v;
    }
    if (!v)
        return TEXT_ZERO;
    *key = canonical(kmer, k) >> 1;
    *count = v;
    return TEXT_OK;
}

} // namespace brx

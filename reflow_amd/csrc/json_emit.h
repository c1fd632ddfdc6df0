// json_emit.h -- internal: the bytes of one Map entry of a Fileset's JSON,
//   "<path>":{"ID":"sha256:<hex>","Size":<n>}
// by the rules of wire.cpp's json_string / marshal_fileset (Go 1.9/1.10
// encoding/json with escapeHTML, eval.go:1961-1967).  __host__ __device__ and
// free of HIP types: compiled into the marshal kernels (k11_cwrite.hip) and
// into the plain C++ executor of a piece stream (marshal_flat.cpp), so the
// source the GPU runs is the source the sanitizer build runs on the CPU.
// Every read of a path is bounded by that path's own length.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_JSON_HD __host__ __device__
#else
#define RF_JSON_HD
#endif

namespace rf {
namespace json {

// Length of the valid UTF-8 sequence at s[i] (s[i] >= 0x80, i < n), 0 if
// invalid: the acceptance ranges of unicode/utf8.DecodeRuneInString.  Never
// reads s[j] for j >= n.
RF_JSON_HD inline uint32_t utf8_seq(const uint8_t* s, uint32_t n, uint32_t i) {
    const uint8_t b0 = s[i];
    uint32_t want;
    uint8_t lo = 0x80, hi = 0xBF;
    if (b0 >= 0xC2 && b0 <= 0xDF) {
        want = 2;
    } else if (b0 >= 0xE0 && b0 <= 0xEF) {
        want = 3;
        if (b0 == 0xE0) lo = 0xA0;
        if (b0 == 0xED) hi = 0x9F;
    } else if (b0 >= 0xF0 && b0 <= 0xF4) {
        want = 4;
        if (b0 == 0xF0) lo = 0x90;
        if (b0 == 0xF4) hi = 0x8F;
    } else {
        return 0;
    }
    if (n - i < want) return 0;
    if (s[i + 1] < lo || s[i + 1] > hi) return 0;
    for (uint32_t j = 2; j < want; ++j)
        if (s[i + j] < 0x80 || s[i + j] > 0xBF) return 0;
    return want;
}

// What the byte at s[i] turns into: the input bytes it consumes (return) and
// the output bytes it makes (*out_n).
//   kind 0: copied raw (`take` bytes); 1: backslash + the byte; 2: \n \r \t;
//   3: a u00XX escape; 4: the escape of U+FFFD; 5: the escape of U+2028 / U+2029
RF_JSON_HD inline uint32_t classify(const uint8_t* s, uint32_t n, uint32_t i, uint32_t* out_n, uint32_t* kind) {
    const uint8_t b = s[i];
    if (b < 0x80) {
        if (b == '"' || b == '\\') {
            *kind = 1;
            *out_n = 2;
        } else if (b == '\n' || b == '\r' || b == '\t') {
            *kind = 2;
            *out_n = 2;
        } else if (b < 0x20 || b == '<' || b == '>' || b == '&') {
            *kind = 3;
            *out_n = 6;
        } else {
            *kind = 0;
            *out_n = 1;
        }
        return 1;
    }
    const uint32_t len = utf8_seq(s, n, i);
    if (len == 0) {  // utf8.RuneError of size 1: one replacement per bad byte
        *kind = 4;
        *out_n = 6;
        return 1;
    }
    if (len == 3 && b == 0xE2 && s[i + 1] == 0x80 && (s[i + 2] == 0xA8 || s[i + 2] == 0xA9)) {
        *kind = 5;
        *out_n = 6;
        return 3;
    }
    *kind = 0;
    *out_n = len;
    return len;
}

RF_JSON_HD inline uint8_t hex_digit(uint32_t v) { return (uint8_t)(v < 10 ? '0' + v : 'a' + (v - 10)); }

// bytes of the quoted, escaped string
RF_JSON_HD inline uint64_t string_len(const uint8_t* s, uint32_t n) {
    uint64_t len = 2;
    for (uint32_t i = 0; i < n;) {
        uint32_t o, k;
        i += classify(s, n, i, &o, &k);
        len += o;
    }
    return len;
}

RF_JSON_HD inline uint8_t* put_string(uint8_t* o, const uint8_t* s, uint32_t n) {
    *o++ = '"';
    for (uint32_t i = 0; i < n;) {
        uint32_t on, k;
        const uint32_t take = classify(s, n, i, &on, &k);
        const uint8_t b = s[i];
        switch (k) {
            case 0:
                for (uint32_t j = 0; j < take; ++j) *o++ = s[i + j];
                break;
            case 1:
                *o++ = '\\';
                *o++ = b;
                break;
            case 2:
                *o++ = '\\';
                *o++ = b == '\n' ? 'n' : b == '\r' ? 'r' : 't';
                break;
            case 3:
                *o++ = '\\';
                *o++ = 'u';
                *o++ = '0';
                *o++ = '0';
                *o++ = hex_digit(b >> 4);
                *o++ = hex_digit(b & 15);
                break;
            case 4:
                *o++ = '\\';
                *o++ = 'u';
                *o++ = 'f';
                *o++ = 'f';
                *o++ = 'f';
                *o++ = 'd';
                break;
            default:  // U+2028 / U+2029
                *o++ = '\\';
                *o++ = 'u';
                *o++ = '2';
                *o++ = '0';
                *o++ = '2';
                *o++ = hex_digit((uint32_t)s[i + 2] - 0xA0);
                break;
        }
        i += take;
    }
    *o++ = '"';
    return o;
}

// decimal int64, INT64_MIN included: the magnitude is taken in uint64
RF_JSON_HD inline uint32_t dec_len(int64_t v) {
    uint64_t m = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    uint32_t d = 1;
    while (m >= 10) {
        m /= 10;
        ++d;
    }
    return d + (v < 0 ? 1u : 0u);
}

RF_JSON_HD inline uint8_t* put_dec(uint8_t* o, int64_t v) {
    uint64_t m = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    const uint32_t n = dec_len(v);
    uint8_t* end = o + n;
    uint8_t* p = end;
    do {
        *--p = (uint8_t)('0' + m % 10);
        m /= 10;
    } while (m);
    if (v < 0) *--p = '-';
    return end;
}

// :{"ID":"sha256: + 64 hex digits + ","Size": + the closing brace
constexpr uint32_t kEntryFixed = 15 + 64 + 9 + 1;

// Bytes of one entry, without the comma a later entry of its Map carries.
RF_JSON_HD inline uint64_t entry_len(const uint8_t* path, uint32_t n, int64_t size) {
    return string_len(path, n) + kEntryFixed + dec_len(size);
}

// Writes [","] + the entry at out; returns the end.
RF_JSON_HD inline uint8_t* emit_entry(uint8_t* out, const uint8_t* path, uint32_t n, const uint8_t* id32, int64_t size,
                                      bool comma) {
    uint8_t* o = out;
    if (comma) *o++ = ',';
    o = put_string(o, path, n);
    const char head[] = ":{\"ID\":\"sha256:";
    for (uint32_t i = 0; i < 15; ++i) *o++ = (uint8_t)head[i];
    for (uint32_t i = 0; i < 32; ++i) {
        *o++ = hex_digit(id32[i] >> 4);
        *o++ = hex_digit(id32[i] & 15);
    }
    const char mid[] = "\",\"Size\":";
    for (uint32_t i = 0; i < 9; ++i) *o++ = (uint8_t)mid[i];
    o = put_dec(o, size);
    *o++ = '}';
    return o;
}

RF_JSON_HD inline bool id_is_zero(const uint8_t* id32) {
    uint8_t acc = 0;
    for (uint32_t i = 0; i < 32; ++i) acc |= id32[i];
    return acc == 0;
}

}  // namespace json
}  // namespace rf

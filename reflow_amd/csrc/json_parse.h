// json_parse.h -- internal: the inverse of json_emit.h.  Reads the canonical
// JSON of a Fileset value -- exactly the bytes json_emit.h / wire.cpp's
// marshal_fileset write (json.Marshal(Fileset), eval.go:1961-1967) -- and
// nothing else: no whitespace, keys in the encoder's case and order, no
// unknown or duplicate fields, no "Fileset":{} or "List":[] (omitempty never
// emits them), no escape the encoder never emits (the u-escape of a letter,
// \/, \b, upper-case hex).  Every other document is refused with a reason mask
// and goes to the caller's tolerant decoder.
//
//   node  := '{' [ '"List":[' node (',' node)* ']' ] [ ',' if both ]
//                [ '"Fileset":{' entry (',' entry)* '}' ] '}'
//   entry := string ':{"ID":"sha256:' 64x[0-9a-f] '","Size":' int '}'
//   int   := '-'? ( '0' | [1-9][0-9]* )      within int64, no "-0"
//
// A string's units are: raw bytes json::classify puts in kind 0; \" \\ \n \r
// \t; the u-escape 00XX (lower-case hex) of a byte classify puts in kind 3;
// the u-escape fffd (decodes to EF BF BD); the u-escapes 2028 and 2029.
// Within a Map the DECODED paths ascend strictly bytewise (the encoder sorts,
// and strict order excludes duplicates).  One consequence: a document made
// from paths with invalid
// UTF-8, whose replacement bytes break that order, is reported as not
// canonical.  An all-zero ID, node nesting above 4096 and an empty document
// are refused, as the marshal refuses them.
//
// Two forms of the same language live here, both __host__ __device__ and free
// of HIP types:
//   * parse_document: one pass, left to right, no stack (bracket types follow
//     from the position, so a depth counter is all the state).  The host form
//     (unmarshal_flat.cpp), and the source of every refused document's reason
//     mask on the device.  The mask names the first thing that is wrong; where
//     the document's end cuts an element short it is kWhyLength.
//   * tile_check_byte / tile_depth_byte: the verdict as a conjunction of
//     per-byte predicates over a bounded neighbourhood, the quote bits and the
//     scanned parity and depth -- what the kernels of k12_unmarshal.hip run,
//     and what unmarshal_flat.cpp can run beside parse_document on the CPU.
// Every read is bounded by the document's own [start, end).
#pragma once
#include "json_emit.h"

namespace rf {
namespace json {

enum : uint32_t {
    kWhyStructure = 1,
    kWhyString = 2,
    kWhyId = 4,
    kWhySize = 8,
    kWhyOrder = 16,
    kWhyDepth = 32,
    kWhyLength = 64
};
constexpr uint32_t kMaxNodeDepth = 4096;  // a root is at depth 0 (marshal_flat.cpp's limit)

RF_JSON_HD inline bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
RF_JSON_HD inline int hex_val(uint8_t c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

// One unit of a string at s[i] (i < n, s[i] is not the closing quote): the
// input bytes it takes (return; 0 = refused, *why set) and its decoded bytes
// (out[0 .. *on), at most 4).
RF_JSON_HD inline uint32_t unit_decode(const uint8_t* s, uint32_t n, uint32_t i, uint8_t* out, uint32_t* on,
                                       uint32_t* why) {
    const uint8_t b = s[i];
    if (b != '\\') {
        if (b >= 0x80 && utf8_seq(s, n, i) == 0) {
            *why = kWhyString;
            return 0;
        }
        uint32_t o, k;
        const uint32_t take = classify(s, n, i, &o, &k);
        if (k != 0) {
            *why = kWhyString;
            return 0;
        }
        for (uint32_t j = 0; j < take; ++j) out[j] = s[i + j];
        *on = take;
        return take;
    }
    if (n - i < 2) {
        *why = kWhyLength;
        return 0;
    }
    const uint8_t c = s[i + 1];
    *on = 1;
    if (c == '"' || c == '\\') {
        out[0] = c;
        return 2;
    }
    if (c == 'n' || c == 'r' || c == 't') {
        out[0] = c == 'n' ? '\n' : c == 'r' ? '\r' : '\t';
        return 2;
    }
    if (c != 'u') {
        *why = kWhyString;
        return 0;
    }
    if (n - i < 6) {
        *why = kWhyLength;
        return 0;
    }
    const uint8_t h0 = s[i + 2], h1 = s[i + 3], h2 = s[i + 4], h3 = s[i + 5];
    if (h0 == '0' && h1 == '0') {
        const int hi = hex_val(h2), lo = hex_val(h3);
        if (hi >= 0 && lo >= 0) {
            const uint8_t v = (uint8_t)(hi * 16 + lo);
            uint32_t o, k;
            (void)classify(&v, 1, 0, &o, &k);
            if (k == 3) {
                out[0] = v;
                return 6;
            }
        }
    } else if (h0 == 'f' && h1 == 'f' && h2 == 'f' && h3 == 'd') {
        out[0] = 0xEF, out[1] = 0xBF, out[2] = 0xBD;
        *on = 3;
        return 6;
    } else if (h0 == '2' && h1 == '0' && h2 == '2' && (h3 == '8' || h3 == '9')) {
        out[0] = 0xE2, out[1] = 0x80, out[2] = (uint8_t)(0xA0 + (h3 - '0'));
        *on = 3;
        return 6;
    }
    *why = kWhyString;
    return 0;
}

// The units of s[b, e) (a string's inside) one decoded byte at a time.
struct PathDec {
    const uint8_t* s;
    uint32_t i, e;
    uint8_t buf[4];
    uint32_t have = 0, pos = 0;
    bool bad = false;
    RF_JSON_HD PathDec(const uint8_t* s_, uint32_t b_, uint32_t e_) : s(s_), i(b_), e(e_) {}
    RF_JSON_HD int next() {
        if (pos < have) return buf[pos++];
        if (i >= e) return -1;
        uint32_t why;
        const uint32_t take = unit_decode(s, e, i, buf, &have, &why);
        if (!take) {
            bad = true;
            have = pos = 0;
            return -1;
        }
        i += take;
        pos = 1;
        return buf[0];
    }
};

// decoded(s[b0, e0)) < decoded(s[b1, e1)) bytewise; false if either does not decode
RF_JSON_HD inline bool path_less(const uint8_t* s, uint32_t b0, uint32_t e0, uint32_t b1, uint32_t e1) {
    PathDec x(s, b0, e0), y(s, b1, e1);
    for (;;) {
        const int cx = x.next(), cy = y.next();
        if (x.bad || y.bad) return false;
        if (cy < 0) return false;  // y ended: x >= y
        if (cx < 0) return true;   // x is a proper prefix
        if (cx != cy) return cx < cy;
    }
}

// Decoded bytes of the string whose inside starts at s[b]: checks every unit up
// to the closing quote.  Returns the quote's index, or 0 with *why set.
RF_JSON_HD inline uint32_t string_scan(const uint8_t* s, uint32_t n, uint32_t b, uint32_t* dec_len, uint32_t* why) {
    uint32_t i = b, len = 0;
    for (;;) {
        if (i >= n) {
            *why = kWhyLength;
            return 0;
        }
        if (s[i] == '"') break;
        uint8_t tmp[4];
        uint32_t on;
        const uint32_t take = unit_decode(s, n, i, tmp, &on, why);
        if (!take) return 0;
        i += take;
        len += on;
    }
    *dec_len = len;
    return i;
}

// decodes s[b, e) (checked before) into out; returns the end of the output
RF_JSON_HD inline uint8_t* path_decode(const uint8_t* s, uint32_t b, uint32_t e, uint8_t* out) {
    for (uint32_t i = b; i < e;) {
        uint32_t on, why;
        const uint32_t take = unit_decode(s, e, i, out, &on, &why);
        if (!take) break;
        i += take;
        out += on;
    }
    return out;
}

// s[*i ..) must be lit[0 .. len): kWhyLength where the document ends first, bit otherwise
RF_JSON_HD inline bool expect(const uint8_t* s, uint32_t n, uint32_t* i, const char* lit, uint32_t len, uint32_t bit,
                              uint32_t* why) {
    for (uint32_t k = 0; k < len; ++k, ++*i) {
        if (*i >= n) {
            *why = kWhyLength;
            return false;
        }
        if (s[*i] != (uint8_t)lit[k]) {
            *why = bit;
            return false;
        }
    }
    return true;
}

// int at s[*i]: '-'? ('0' | [1-9][0-9]*) within int64; stops after its last digit
RF_JSON_HD inline bool parse_int(const uint8_t* s, uint32_t n, uint32_t* i, int64_t* v, uint32_t* why) {
    bool neg = false;
    if (*i < n && s[*i] == '-') {
        neg = true;
        ++*i;
    }
    if (*i >= n) {
        *why = kWhyLength;
        return false;
    }
    if (!is_digit(s[*i])) {
        *why = kWhySize;
        return false;
    }
    if (s[*i] == '0') {
        ++*i;
        if (neg) {
            *why = kWhySize;  // -0
            return false;
        }
        *v = 0;
        return true;  // (a digit after it is not the entry's closing brace)
    }
    const uint64_t limit = neg ? (1ull << 63) : (1ull << 63) - 1;
    uint64_t m = 0;
    while (*i < n && is_digit(s[*i])) {
        const uint32_t d = s[*i] - '0';
        if (m > (limit - d) / 10) {
            *why = kWhySize;
            return false;
        }
        m = m * 10 + d;
        ++*i;
    }
    *v = neg ? (int64_t)(0 - m) : (int64_t)m;
    return true;
}

// The entry's text after its path's closing quote, from s[i]:
//   :{"ID":"sha256:<64 hex>","Size":<int>}
// Returns the index after the closing brace, or 0 with *why set.
RF_JSON_HD inline uint32_t parse_entry_tail(const uint8_t* s, uint32_t n, uint32_t i, uint8_t* id32, int64_t* size,
                                            uint32_t* why) {
    if (!expect(s, n, &i, ":{\"ID\":\"", 8, kWhyStructure, why)) return 0;
    if (!expect(s, n, &i, "sha256:", 7, kWhyId, why)) return 0;
    uint8_t any = 0;
    for (uint32_t k = 0; k < 32; ++k) {
        int v[2];
        for (uint32_t h = 0; h < 2; ++h, ++i) {
            if (i >= n) {
                *why = kWhyLength;
                return 0;
            }
            if ((v[h] = hex_val(s[i])) < 0) {
                *why = kWhyId;
                return 0;
            }
        }
        id32[k] = (uint8_t)(v[0] * 16 + v[1]);
        any |= id32[k];
    }
    if (!expect(s, n, &i, "\"", 1, kWhyId, why)) return 0;
    if (!any) {
        *why = kWhyId;  // digest.Digest's zero text form is unpinned: the marshal refuses it too
        return 0;
    }
    if (!expect(s, n, &i, ",\"Size\":", 8, kWhyStructure, why)) return 0;
    if (!parse_int(s, n, &i, size, why)) return 0;
    if (!expect(s, n, &i, "}", 1, kWhySize, why)) return 0;
    return i;
}

// ---- the sequential form -----------------------------------------------------------
// Sink: entry(path_begin, path_end, decoded_len, id32, size) in document order
// (path = the string's inside, still escaped) and node(depth) at every node's
// closing brace.  Nodes therefore come in closing order (post-order), and the
// entries since the previous node() are the closing node's Map.
struct NullSink {
    RF_JSON_HD void entry(uint32_t, uint32_t, uint32_t, const uint8_t*, int64_t) {}
    RF_JSON_HD void node(uint32_t) {}
};

// Returns 0 when s[0, n) is canonical, else the reason mask.
template <class Sink>
RF_JSON_HD inline uint32_t parse_document(const uint8_t* s, uint32_t n, Sink& sink) {
    uint32_t i = 0, depth = 0, why = 0;
    if (n == 0) return kWhyLength;
    for (;;) {
        // a node's opening brace
        if (i >= n) return kWhyLength;
        if (s[i] != '{') return kWhyStructure;
        if (depth > kMaxNodeDepth) return kWhyDepth;
        ++i;
        if (i >= n) return kWhyLength;
        bool map = false;
        if (s[i] == '"') {
            if (i + 1 >= n) return kWhyLength;
            if (s[i + 1] == 'L') {
                if (!expect(s, n, &i, "\"List\":[", 8, kWhyStructure, &why)) return why;
                ++depth;
                continue;
            }
            map = true;
        }
        for (;;) {
            if (map) {
                if (!expect(s, n, &i, "\"Fileset\":{", 11, kWhyStructure, &why)) return why;
                uint32_t pb = 0, pe = 0;
                for (bool first = true;; first = false) {
                    if (i >= n) return kWhyLength;
                    if (s[i] != '"') return kWhyStructure;
                    uint32_t dec;
                    const uint32_t q = string_scan(s, n, i + 1, &dec, &why);
                    if (!q) return why;
                    if (!first && !path_less(s, pb, pe, i + 1, q)) return kWhyOrder;
                    pb = i + 1;
                    pe = q;
                    uint8_t id[32];
                    int64_t size;
                    i = parse_entry_tail(s, n, q + 1, id, &size, &why);
                    if (!i) return why;
                    sink.entry(pb, pe, dec, id, size);
                    if (i >= n) return kWhyLength;
                    if (s[i] == ',') {
                        ++i;
                        continue;
                    }
                    if (s[i] != '}') return kWhyStructure;
                    ++i;
                    break;
                }
            }
            // the node's closing brace
            if (i >= n) return kWhyLength;
            if (s[i] != '}') return kWhyStructure;
            ++i;
            sink.node(depth);
            if (depth == 0) return i == n ? 0u : (uint32_t)kWhyStructure;
            if (i >= n) return kWhyLength;
            if (s[i] == ',') {  // the List's next node
                ++i;
                break;
            }
            if (s[i] != ']') return kWhyStructure;
            ++i;
            --depth;
            if (i >= n) return kWhyLength;
            map = s[i] == ',';
            if (map) ++i;
        }
    }
}

// ---- the per-byte form -------------------------------------------------------------
// s is the arena, [ds, de) one document in it (de > ds), qm the quote bits of
// the arena: bit (j & 15) of qm[j >> 4] is set where s[j] is a '"' that an even
// run of backslashes (counted back to ds at most) precedes.
RF_JSON_HD inline bool qbit(const uint16_t* qm, uint32_t j) { return (qm[j >> 4] >> (j & 15)) & 1; }

RF_JSON_HD inline bool quote_is_delim(const uint8_t* s, uint32_t ds, uint32_t i) {
    uint32_t run = 0;
    for (uint32_t j = i; j > ds && s[j - 1] == '\\'; --j) ++run;
    return (run & 1) == 0;
}

// the last quote bit in [ds, j), or -1; whole empty words are skipped
RF_JSON_HD inline int64_t prev_delim(const uint16_t* qm, uint32_t ds, uint32_t j) {
    while (j > ds) {
        --j;
        if ((j & 15) == 15 && j - ds >= 15 && qm[j >> 4] == 0) {
            j -= 15;
            continue;
        }
        if (qbit(qm, j)) return j;
    }
    return -1;
}

enum : uint32_t { kTokBad = 0, kTokNodeOpen, kTokMapOpen, kTokEntryOpen, kTokEntryClose, kTokMapClose, kTokNodeClose };

// A '{' outside strings: an entry's when "ID":" follows, else a Map's when a
// colon precedes, else a node's.
RF_JSON_HD inline uint32_t open_kind(const uint8_t* s, uint32_t ds, uint32_t de, uint32_t i) {
    if (de - i > 6 && s[i + 1] == '"' && s[i + 2] == 'I' && s[i + 3] == 'D' && s[i + 4] == '"' && s[i + 5] == ':' &&
        s[i + 6] == '"')
        return kTokEntryOpen;
    if (i > ds && s[i - 1] == ':') return kTokMapOpen;
    return kTokNodeOpen;
}

// A '}' outside strings, by the token before it: after a digit it closes an
// entry, after an entry's close a Map, after a Map's close, a ']' or a node's
// own '{' a node; a fourth in a row is never legal.
RF_JSON_HD inline uint32_t close_kind(const uint8_t* s, uint32_t ds, uint32_t de, uint32_t i) {
    uint32_t p = i, run = 0;
    while (run < 3 && p > ds && s[p - 1] == '}') {
        --p;
        ++run;
    }
    if (p == ds) return kTokBad;
    const uint8_t c = s[p - 1];
    if (is_digit(c)) return run == 0 ? kTokEntryClose : run == 1 ? kTokMapClose : run == 2 ? kTokNodeClose : kTokBad;
    if (run == 0 && (c == ']' || (c == '{' && open_kind(s, ds, de, p - 1) == kTokNodeOpen))) return kTokNodeClose;
    return kTokBad;
}

// +1 at a node's '{' and a List's '[', -1 at their closers; s[i] is outside strings
RF_JSON_HD inline int32_t depth_delta(const uint8_t* s, uint32_t ds, uint32_t de, uint32_t i) {
    const uint8_t c = s[i];
    if (c == '[') return 1;
    if (c == ']') return -1;
    if (c == '{') return open_kind(s, ds, de, i) == kTokNodeOpen ? 1 : 0;
    if (c == '}') return close_kind(s, ds, de, i) == kTokNodeClose ? -1 : 0;
    return 0;
}

// s[i] closes a path (a string that ':' and an entry's '{' follow)
RF_JSON_HD inline bool closes_path(const uint8_t* s, uint32_t ds, uint32_t de, uint32_t i) {
    return de - i > 2 && s[i + 1] == ':' && s[i + 2] == '{' && open_kind(s, ds, de, i + 2) == kTokEntryOpen;
}

struct ByteCounts {
    int32_t ddepth = 0;
    uint32_t nodes = 0, entries = 0, path_bytes = 0;
};

RF_JSON_HD inline bool lit_is(const uint8_t* s, uint32_t b, uint32_t e, const char* lit, uint32_t len) {
    if (e - b != len) return false;
    for (uint32_t k = 0; k < len; ++k)
        if (s[b + k] != (uint8_t)lit[k]) return false;
    return true;
}

// The lane of a string's closing quote at s[i]: the string's place (what stands
// before its opening quote, what follows its closing one) fixes what it must
// be.  A path's lane checks its units, the entry's text behind it, and its
// order against the Map's previous path.
RF_JSON_HD inline bool string_lane(const uint8_t* s, const uint16_t* qm, uint32_t ds, uint32_t de, uint32_t i,
                                   ByteCounts* o) {
    enum { L_NODE, L_MAP, L_ENTRY, L_NEXT, L_LISTEND, L_SIZE, L_COLON };
    const int64_t oq = prev_delim(qm, ds, i);
    if (oq <= (int64_t)ds) return false;
    const uint32_t q0 = (uint32_t)oq, b = q0 + 1;
    int left;
    const uint8_t pc = s[q0 - 1];
    if (pc == '{') {
        const uint32_t k = open_kind(s, ds, de, q0 - 1);
        left = k == kTokNodeOpen ? L_NODE : k == kTokMapOpen ? L_MAP : L_ENTRY;
    } else if (pc == ',') {
        if (q0 - ds < 2) return false;
        const uint8_t p2 = s[q0 - 2];
        if (p2 == '}') {
            if (close_kind(s, ds, de, q0 - 2) != kTokEntryClose) return false;
            left = L_NEXT;
        } else if (p2 == ']') {
            left = L_LISTEND;
        } else if (p2 == '"') {
            left = L_SIZE;
        } else {
            return false;
        }
    } else if (pc == ':') {
        left = L_COLON;
    } else {
        return false;
    }
    if (de - i < 2) return false;
    if (s[i + 1] == ',') return left == L_COLON;  // the digest: its entry's lane reads it
    if (s[i + 1] != ':' || de - i < 3) return false;
    const uint8_t c2 = s[i + 2];
    if (c2 == '[') return left == L_NODE && lit_is(s, b, i, "List", 4);
    if (c2 == '"') return left == L_ENTRY && lit_is(s, b, i, "ID", 2);
    if (c2 == '-' || is_digit(c2)) return left == L_SIZE && lit_is(s, b, i, "Size", 4);
    if (c2 != '{') return false;
    if (open_kind(s, ds, de, i + 2) != kTokEntryOpen)
        return (left == L_NODE || left == L_LISTEND) && lit_is(s, b, i, "Fileset", 7);
    if (left != L_MAP && left != L_NEXT) return false;
    uint32_t dec = 0, why = 0;
    for (uint32_t j = b; j < i;) {  // every unit inside [b, i)
        uint8_t tmp[4];
        uint32_t on;
        const uint32_t take = unit_decode(s, i, j, tmp, &on, &why);
        if (!take) return false;
        j += take;
        dec += on;
    }
    uint8_t id[32];
    int64_t size;
    if (!parse_entry_tail(s, de, i + 1, id, &size, &why)) return false;
    if (left == L_NEXT) {  // the previous entry's path: eight quote bits back
        int64_t q = q0;
        uint32_t pe = 0;
        for (int k = 0; k < 8; ++k) {
            q = prev_delim(qm, ds, (uint32_t)q);
            if (q < 0) return false;
            if (k == 6) pe = (uint32_t)q;
        }
        if (!path_less(s, (uint32_t)q + 1, pe, b, i)) return false;
    }
    o->entries = 1;
    o->path_bytes = dec;
    return true;
}

// Everything about s[i] that needs no depth; pb = an odd number of quote bits
// in [ds, i).  The document is canonical iff every byte passes here and in
// tile_depth_byte.
RF_JSON_HD inline bool tile_check_byte(const uint8_t* s, const uint16_t* qm, uint32_t ds, uint32_t de, uint32_t i,
                                       bool pb, ByteCounts* o) {
    const uint8_t c = s[i];
    const bool q = c == '"' && qbit(qm, i);
    const bool first = i == ds, last = i + 1 == de;
    if (first && c != '{') return false;
    if (last && (c != '}' || pb)) return false;
    if (pb && !q) return true;  // inside a string: the string's lane reads it
    const uint8_t pv = first ? 0 : s[i - 1], nx = last ? 0 : s[i + 1];
    switch (c) {
        case '{': {
            const uint32_t k = open_kind(s, ds, de, i);
            if (k == kTokNodeOpen) {
                o->ddepth = 1;
                return (first || pv == '[' || pv == ',') && (nx == '}' || nx == '"');
            }
            return pv == ':' && nx == '"';
        }
        case '[':
            o->ddepth = 1;
            return pv == ':' && nx == '{';
        case ':':
            return pv == '"' && (nx == '[' || nx == '{' || nx == '"' || nx == '-' || is_digit(nx));
        case ',':
            if (pv == '}') {
                const uint32_t k = close_kind(s, ds, de, i - 1);
                return k == kTokNodeClose ? nx == '{' : k == kTokEntryClose ? nx == '"' : false;
            }
            return (pv == ']' || pv == '"') && nx == '"';
        case ']':
            o->ddepth = -1;
            return pv == '}' && close_kind(s, ds, de, i - 1) == kTokNodeClose && (nx == ',' || nx == '}');
        case '}': {
            const uint32_t k = close_kind(s, ds, de, i);
            if (k == kTokEntryClose) return nx == ',' || nx == '}';
            if (k == kTokMapClose) return nx == '}';
            if (k != kTokNodeClose) return false;
            o->ddepth = -1;
            o->nodes = 1;
            return last || nx == ',' || nx == ']';
        }
        case '-':
            return pv == ':' && is_digit(nx);
        case '"':
            if (!q) return false;
            if (!pb) return pv == '{' || pv == ',' || pv == ':';
            return string_lane(s, qm, ds, de, i, o);
        default:
            if (is_digit(c)) return (pv == ':' || pv == '-' || is_digit(pv)) && (is_digit(nx) || nx == '}');
            return false;
    }
}

// The depth rules at s[i] (outside strings, not a quote); depth = the sum of
// depth_delta over [ds, i).  Node braces sit at even depth, List brackets at
// odd depth, the depth is zero after the last byte and nowhere before, and no
// node lies deeper than kMaxNodeDepth.  With the bracket types fixed by that
// parity, a balanced depth means the brackets match by type.
RF_JSON_HD inline bool tile_depth_byte(const uint8_t* s, uint32_t ds, uint32_t de, uint32_t i, int32_t depth) {
    const int32_t d = depth_delta(s, ds, de, i);
    if (d == 0) return true;
    if (depth < 0) return false;
    if (s[i] == '{') return (depth & 1) == 0 && (uint32_t)depth / 2 <= kMaxNodeDepth && (depth == 0) == (i == ds);
    if (s[i] == '[') return (depth & 1) == 1;
    if (s[i] == ']') return (depth & 1) == 0 && depth >= 2;
    return (depth & 1) == 1 && (depth == 1) == (i + 1 == de);
}

}  // namespace json
}  // namespace rf

// include/suffix_table.hpp -- C++ host-side mirror of the reference's public
// type `SuffixTable` (/root/reference/src/table.rs:54-294) on top of the C ABI
// (suffix_hip.h).  Header-only; link with -lsuffix_hip.  The reference is
// compiled code (Rust) and this image has no Rust toolchain, so this is the
// compiled-language host side; rust/suffix-hip/src/lib.rs shows the Rust binding.
//
// Same names, argument meaning and error behaviour as the Rust API:
//   new_ / new_naive (doc-hidden upstream, :93-100: the definition, sorted on the host -- the reference's own test oracle,
//   tests/tests.rs:18-20; never a fallback of new_) / from_parts / into_parts / lcp_lens / table / text / len / is_empty /
//   suffix / suffix_bytes / contains / positions / any_position,
// plus the additive positions_batch / contains_batch, repeat_lens / repeated_spans, bwt / unbwt, lz77 / unlz, mems, approx_positions,
// inverse_table / lce / lcp_range_min, runs / lyndon_array / lyndon_factorization and fm_index (class FmIndex below: the same queries from the transform alone).  Errors that are panics
// in the reference (assert! :380, assert_eq! :117) are std::runtime_error /
// std::length_error here.  Text is indexed by BYTES (:379).
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "suffix_hip.h"

namespace suffix {

class SuffixTable {
public:
    // SuffixTable::new (:78-85): builds the table on the GPU.
    static SuffixTable new_(std::string text)
    {
        SuffixTable st;
        st.text_ = std::move(text);
        st.table_.assign(st.text_.size(), 0u);                       // vec![0u32; n] (:381)
        check(sfx_build_sa_u32(bytes(st.text_), st.text_.size(), st.table_.data()), "SuffixTable::new");
        return st;
    }
    // SuffixTable::new_naive (:93-100, #[doc(hidden)]) -> naive_table (:367-376): the definition -- all byte suffixes sorted by
    // comparison on the host, O(n^2 log n).  Upstream keeps it as the oracle of its own tests (tests/tests.rs:18-20); it is the same
    // here: what a caller compares new_() against, never something new_() falls back to.
    static SuffixTable new_naive(std::string text)
    {
        SuffixTable st;
        st.text_ = std::move(text);
        if (st.text_.size() > 0xFFFFFFFFull) throw std::length_error("SuffixTable::new_naive: text longer than u32::MAX");
        st.table_.resize(st.text_.size());
        for (size_t i = 0; i < st.table_.size(); i++) st.table_[i] = (uint32_t)i;
        const std::string_view t(st.text_);
        std::sort(st.table_.begin(), st.table_.end(), [t](uint32_t a, uint32_t b) { return t.substr(a) < t.substr(b); });
        return st;
    }
    // SuffixTable::from_parts (:111-119): unchecked except for the lengths.
    static SuffixTable from_parts(std::string text, std::vector<uint32_t> table)
    {
        if (text.size() != table.size()) throw std::length_error("text.len() != table.len()");   // :117
        SuffixTable st;
        st.text_ = std::move(text);
        st.table_ = std::move(table);
        return st;
    }
    std::pair<std::string, std::vector<uint32_t>> into_parts() && { return {std::move(text_), std::move(table_)}; }

    SuffixTable(SuffixTable&& o) noexcept { *this = std::move(o); }
    SuffixTable& operator=(SuffixTable&& o) noexcept
    {
        text_ = std::move(o.text_);
        table_ = std::move(o.table_);
        lazy_ = std::move(o.lazy_);
        o.lazy_ = std::make_unique<LazyIndex>();
        return *this;
    }
    SuffixTable(const SuffixTable& o) : text_(o.text_), table_(o.table_) {}      // derive(Clone)
    ~SuffixTable() = default;
    bool operator==(const SuffixTable& o) const { return text_ == o.text_ && table_ == o.table_; }   // :54

    // lcp_lens (:130-138)
    std::vector<uint32_t> lcp_lens() const
    {
        std::vector<uint32_t> lcp(table_.size(), 0u);
        check(sfx_build_lcp_u32(bytes(text_), text_.size(), table_.data(), lcp.data()), "lcp_lens");
        return lcp;
    }
    const std::vector<uint32_t>& table() const { return table_; }     // :142
    const std::string& text() const { return text_; }                 // :148
    size_t len() const { return table_.size(); }                      // :156
    bool is_empty() const { return table_.empty(); }                  // :162
    std::string_view suffix(size_t i) const { return std::string_view(text_).substr(table_.at(i)); }   // :168
    std::string_view suffix_bytes(size_t i) const { return suffix(i); }                                  // :174

    // positions (:223-259): the occurrences of `query`, in suffix-array order,
    // as a view into table().
    std::pair<const uint32_t*, const uint32_t*> positions(std::string_view query) const
    {
        if (text_.empty() || query.empty()) return {table_.data(), table_.data()};   // :228-229
        auto se = positions_batch({query});
        return {table_.data() + se[0].first, table_.data() + se[0].second};
    }
    // any_position (:279-293); which occurrence is arbitrary by contract (:261-262)
    std::optional<uint32_t> any_position(std::string_view query) const
    {
        if (query.empty() || text_.empty()) return std::nullopt;
        uint64_t off[2] = {0, query.size()};
        uint8_t found = 0;
        uint32_t pos = 0;
        check(sfx_contains_batch(index(), reinterpret_cast<const uint8_t*>(query.data()), off, 1, &found, &pos),
              "any_position");
        if (!found) return std::nullopt;
        return pos;
    }
    bool contains(std::string_view query) const { return any_position(query).has_value(); }   // :197-199

    // additive: many queries in one launch; (start, end) index pairs into table()
    std::vector<std::pair<uint32_t, uint32_t>> positions_batch(const std::vector<std::string_view>& qs) const
    {
        std::vector<uint64_t> off(qs.size() + 1, 0);
        std::string blob;
        for (size_t k = 0; k < qs.size(); k++) { blob.append(qs[k]); off[k + 1] = blob.size(); }
        std::vector<uint32_t> s(qs.size()), e(qs.size());
        if (!qs.empty())
            check(sfx_positions_batch(index(), reinterpret_cast<const uint8_t*>(blob.data()), off.data(), qs.size(),
                                      s.data(), e.data()), "positions_batch");
        std::vector<std::pair<uint32_t, uint32_t>> out(qs.size());
        for (size_t k = 0; k < qs.size(); k++) out[k] = {s[k], e[k]};
        return out;
    }

    // additive: rep[p] = the longest common prefix of the suffix at byte p with any other suffix (SFX_REP_ANY) or with any
    // suffix that starts earlier (SFX_REP_EARLIER: the longest-previous-factor array), see suffix_hip.h
    std::vector<uint32_t> repeat_lens(int scope = SFX_REP_ANY) const
    {
        if (scope != SFX_REP_ANY && scope != SFX_REP_EARLIER) throw std::invalid_argument("repeat_lens: scope must be SFX_REP_ANY or SFX_REP_EARLIER");
        const std::vector<uint32_t> lcp = lcp_lens();
        std::vector<uint32_t> rep(table_.size(), 0u);
        check(sfx_repeat_lens_u32(table_.data(), lcp.data(), nullptr, table_.size(), scope, rep.data(), nullptr), "repeat_lens");
        return rep;
    }
    // additive: [begin, end) of the maximal runs of bytes inside a repeat of at least min_len bytes, ascending
    std::vector<std::pair<uint32_t, uint32_t>> repeated_spans(uint32_t min_len, int scope = SFX_REP_ANY) const
    {
        if (min_len == 0) throw std::invalid_argument("repeated_spans: min_len must be at least 1");
        const std::vector<uint32_t> rep = repeat_lens(scope);
        const uint64_t cap = rep.size() / min_len + 1;                               // every run is at least min_len long
        std::vector<uint32_t> b(cap), e(cap);
        uint64_t count = 0;
        check(sfx_repeat_spans_u32(rep.data(), rep.size(), min_len, nullptr, 0, b.data(), e.data(), cap, &count), "repeated_spans");
        std::vector<std::pair<uint32_t, uint32_t>> out((size_t)count);
        for (size_t k = 0; k < out.size(); k++) out[k] = {b[k], e[k]};
        return out;
    }

    // additive: matching statistics of a second text against this one (suffix_hip.h): len[i] = the longest prefix of
    // query[i..] (at most max_len bytes, 0 = no cap) that occurs in the text, src[i] = one position where it stands
    // (UINT32_MAX where len[i] == 0; which occurrence is arbitrary).  The cost grows with the lengths found.
    struct MatchStats { std::vector<uint32_t> len, src; };
    MatchStats match_stats(std::string_view query, uint32_t max_len = 0) const
    {
        MatchStats ms{std::vector<uint32_t>(query.size(), 0u), std::vector<uint32_t>(query.size(), 0xFFFFFFFFu)};
        if (!query.empty() && !text_.empty())
            check(sfx_index_match_stats(index(), reinterpret_cast<const uint8_t*>(query.data()), query.size(), max_len, ms.len.data(),
                                        ms.src.data(), nullptr, nullptr), "match_stats");
        return ms;
    }
    // additive: [begin, end) in query coordinates, ascending: the maximal runs of query bytes inside a stretch of at least
    // min_len bytes that also occurs in the text -- the search capped at min_len, then the span report of the repeats
    std::vector<std::pair<uint32_t, uint32_t>> shared_spans(std::string_view query, uint32_t min_len) const
    {
        if (min_len == 0) throw std::invalid_argument("shared_spans: min_len must be at least 1");
        return spans_of(match_stats(query, min_len).len, min_len);
    }
    // additive: the maximal exact matches of at least min_len bytes between a second text and this one (suffix_hip.h,
    // sfx_index_mems): query[qpos .. qpos + len) == text[tpos .. tpos + len), extendable neither to the left nor to the
    // right; ascending by qpos, then by the table rank of tpos.  unique: only matches whose bytes occur once in the text.
    // pairs = the candidate pairs the call looked at; more than max_pairs of them throw std::runtime_error naming the
    // count (a shared stretch of M bytes is M - min_len + 1 pairs; two copies of a^n about n^2 / 2).
    struct Mems {
        std::vector<uint32_t> qpos, tpos, len;
        uint64_t pairs = 0;
        size_t size() const { return len.size(); }
    };
    Mems mems(std::string_view query, uint32_t min_len, bool unique = false, uint64_t max_pairs = 1ull << 30) const
    {
        if (min_len == 0 || max_pairs == 0) throw std::invalid_argument("mems: min_len and max_pairs must be at least 1");
        Mems r;
        if (query.empty() || text_.empty()) return r;
        uint64_t cap = query.size() < 1024 ? 1024 : query.size(), z = 0;
        for (int round = 0; round < 2; round++) {                                    // the room is a guess: once more when there were more
            r.qpos.resize((size_t)cap);
            r.tpos.resize((size_t)cap);
            r.len.resize((size_t)cap);
            check(sfx_index_mems(index(), reinterpret_cast<const uint8_t*>(query.data()), query.size(), min_len, unique ? SFX_MEM_UNIQUE : 0u,
                                 max_pairs, r.qpos.data(), r.tpos.data(), r.len.data(), cap, &r.pairs, &z), "mems");
            if (r.pairs > max_pairs)
                throw std::runtime_error("mems: " + std::to_string(r.pairs) + " candidate pairs exceed max_pairs = " + std::to_string(max_pairs));
            if (z <= cap) break;
            cap = z;
        }
        r.qpos.resize((size_t)z);
        r.tpos.resize((size_t)z);
        r.len.resize((size_t)z);
        return r;
    }
    // additive: where does a pattern occur if up to `mismatches` (<= 255) bytes may differ -- Hamming distance, no
    // insertions or deletions (suffix_hip.h, sfx_index_hamming)?  (position, differing bytes) per occurrence, ascending by
    // position; an empty pattern has none, a pattern of at most `mismatches` bytes occurs wherever it has room.  The work
    // grows with the exact hits of the pattern's mismatches + 1 pieces: more than max_candidates of them throw
    // std::runtime_error naming the count.
    std::vector<std::pair<uint32_t, uint8_t>> approx_positions(std::string_view query, uint32_t mismatches,
                                                               uint64_t max_candidates = 1ull << 30) const
    {
        if (mismatches > 255 || max_candidates == 0) throw std::invalid_argument("approx_positions: mismatches must be at most 255, max_candidates at least 1");
        std::vector<std::pair<uint32_t, uint8_t>> out;
        if (query.empty() || text_.empty()) return out;
        const uint64_t off[2] = {0, query.size()};
        std::vector<uint32_t> pat, tpos;
        std::vector<uint8_t> mism;
        uint64_t cap = 1024, cands = 0, z = 0;
        for (int round = 0; round < 2; round++) {                                    // the room is a guess: once more when there were more
            pat.resize((size_t)cap);
            tpos.resize((size_t)cap);
            mism.resize((size_t)cap);
            check(sfx_index_hamming(index(), reinterpret_cast<const uint8_t*>(query.data()), off, 1, mismatches, max_candidates, pat.data(),
                                    tpos.data(), mism.data(), cap, nullptr, &cands, &z), "approx_positions");
            if (cands > max_candidates)
                throw std::runtime_error("approx_positions: " + std::to_string(cands) + " candidates exceed max_candidates = " +
                                         std::to_string(max_candidates));
            if (z <= cap) break;
            cap = z;
        }
        out.resize((size_t)z);
        for (size_t i = 0; i < out.size(); i++) out[i] = {tpos[i], mism[i]};
        std::sort(out.begin(), out.end());
        return out;
    }
    // additive: longest common extensions between two positions of this text (suffix_hip.h, sfx_lce_*).  inverse_table():
    // isa[table()[r]] = r; throws std::runtime_error for a table (from_parts) that is no permutation.  lce(i, j, k): how
    // far the suffixes at i and j agree when up to k bytes may differ, never past the end of the text; a position equal
    // to len() gives 0, one above 0xFFFFFFFF.  lcp_range_min(lo, hi): min lcp_lens()[lo .. hi), 0xFFFFFFFF for an empty
    // range or hi > len().  The handle (inverse table + min-tree over lcp_lens()) is made on the first call.
    std::vector<uint32_t> inverse_table() const
    {
        std::vector<uint32_t> isa(table_.size());
        check(sfx_inverse_table_u32(table_.data(), table_.size(), isa.data()), "inverse_table");
        return isa;
    }
    std::vector<uint32_t> lce_batch(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, uint32_t mismatches = 0) const
    {
        if (a.size() != b.size()) throw std::invalid_argument("lce_batch: one position of each list per pair");
        std::vector<uint32_t> len(a.size());
        if (!a.empty()) check(sfx_lce_query(lce_index(), a.data(), b.data(), a.size(), mismatches, len.data()), "lce_batch");
        return len;
    }
    uint32_t lce(uint32_t i, uint32_t j, uint32_t mismatches = 0) const { return lce_batch({i}, {j}, mismatches)[0]; }
    std::vector<uint32_t> lcp_range_min_batch(const std::vector<uint32_t>& lo, const std::vector<uint32_t>& hi) const
    {
        if (lo.size() != hi.size()) throw std::invalid_argument("lcp_range_min_batch: one bound of each list per range");
        std::vector<uint32_t> out(lo.size());
        if (!lo.empty()) check(sfx_lce_range_min(lce_index(), lo.data(), hi.data(), lo.size(), out.data()), "lcp_range_min_batch");
        return out;
    }
    uint32_t lcp_range_min(uint32_t lo, uint32_t hi) const { return lcp_range_min_batch({lo}, {hi})[0]; }
    // the spans of a rep-shaped array (repeat_lens, match_stats().len) at min_len >= 1
    static std::vector<std::pair<uint32_t, uint32_t>> spans_of(const std::vector<uint32_t>& rep, uint32_t min_len)
    {
        if (min_len == 0) throw std::invalid_argument("spans_of: min_len must be at least 1");
        const uint64_t cap = rep.size() / min_len + 1;                               // every run is at least min_len long
        std::vector<uint32_t> b(cap), e(cap);
        uint64_t count = 0;
        check(sfx_repeat_spans_u32(rep.data(), rep.size(), min_len, nullptr, 0, b.data(), e.data(), cap, &count), "spans_of");
        std::vector<std::pair<uint32_t, uint32_t>> out((size_t)count);
        for (size_t k = 0; k < out.size(); k++) out[k] = {b[k], e[k]};
        return out;
    }

    // additive: the Burrows-Wheeler transform with sampled ranks (suffix_hip.h): bwt = the last column of the sorted rotations
    // of text$ without its $ entry; samples[k] = the row of the suffix at k * sample_step (samples[0] = the primary row;
    // sample_step 0: the primary only).  sample_step is 0 or a power of two.
    struct Bwt { std::string bwt; std::vector<uint32_t> samples; };
    Bwt bwt(uint32_t sample_step = 256) const
    {
        if (sample_step & (sample_step - 1u)) throw std::invalid_argument("bwt: sample_step must be 0 or a power of two");
        Bwt out{std::string(text_.size(), '\0'), std::vector<uint32_t>((size_t)sfx_bwt_sample_count(text_.size(), sample_step), 0u)};
        if (!text_.empty())
            check(sfx_bwt_u32(bytes(text_), text_.size(), table_.data(), sample_step, reinterpret_cast<uint8_t*>(&out.bwt[0]),
                              out.samples.data()), "bwt");
        return out;
    }
    // ... and its inverse: the text whose transform (bwt, samples) is.  A pair that is the transform of no text throws
    // std::runtime_error -- the walks check themselves, so what is returned is the text.
    static std::string unbwt(std::string_view bwt, const std::vector<uint32_t>& samples, uint32_t sample_step)
    {
        std::string out(bwt.size(), '\0');
        check(sfx_unbwt(reinterpret_cast<const uint8_t*>(bwt.data()), bwt.size(), samples.data(), samples.size(), sample_step,
                        reinterpret_cast<uint8_t*>(&out[0])), "unbwt");
        return out;
    }
    // additive: the greedy LZ77 factorization (suffix_hip.h, sfx_lz77_u32): one entry per phrase.  A copy repeats len bytes
    // from position src < its own begin (it may run into itself) and has lit 0; a literal has len 1, src UINT32_MAX and
    // its byte in lit.  min_len >= 1: shorter repeats become literals; 1 is the classical parse.  size() = z.
    struct Lz77 {
        std::vector<uint32_t> begin, len, src;
        std::string lit;
        size_t size() const { return len.size(); }
    };
    Lz77 lz77(uint32_t min_len = 1) const
    {
        if (min_len == 0) throw std::invalid_argument("lz77: min_len must be at least 1");
        const size_t n = text_.size();
        Lz77 f{std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::string(n, '\0')};
        uint64_t z = 0;
        if (n)
            check(sfx_lz77_u32(bytes(text_), n, table_.data(), nullptr, min_len, f.begin.data(), f.len.data(), f.src.data(),
                               reinterpret_cast<uint8_t*>(&f.lit[0]), n, &z), "lz77");
        f.begin.resize((size_t)z);
        f.len.resize((size_t)z);
        f.src.resize((size_t)z);
        f.lit.resize((size_t)z);
        return f;
    }
    // ... and its decoder: the text of the phrases (len, src, lit).  A list that is no factorization -- a zero length, a
    // literal of another length than 1, a copy that does not point backwards -- throws std::runtime_error.
    static std::string unlz(const std::vector<uint32_t>& len, const std::vector<uint32_t>& src, std::string_view lit)
    {
        if (src.size() != len.size() || lit.size() != len.size()) throw std::invalid_argument("unlz: one entry per phrase");
        uint64_t n = 0;
        for (uint32_t l : len) n += l;
        if (n > 0xFFFFFFFFull) throw std::length_error("unlz: more than u32::MAX bytes");
        std::string out((size_t)n, '\0');
        check(sfx_unlz(len.data(), src.data(), reinterpret_cast<const uint8_t*>(lit.data()), len.size(), n,
                       reinterpret_cast<uint8_t*>(&out[0])), "unlz");
        return out;
    }
    // additive: the maximal repetitions (runs) of the text -- its tandem repeats -- and the Lyndon array (suffix_hip.h,
    // sfx_runs_u32 / sfx_lyndon_array_u32).  runs(): one entry per (begin, end, period) with period the smallest period of
    // text[begin..end), end - begin >= 2 period, extendable to neither side; ascending by (begin, period); kept when
    // min_period <= period <= max_period (0: no limit) and end - begin >= min_len.  lyndon_array(order): the length of the
    // longest Lyndon word starting at every byte under byte order (0) or reversed byte order (1); lyndon_factorization():
    // the starts of the Lyndon factors.
    struct Runs {
        std::vector<uint32_t> begin, end, period;
        size_t size() const { return begin.size(); }
        double exponent(size_t k) const { return (double)(end[k] - begin[k]) / (double)period[k]; }
    };
    Runs runs(uint32_t min_period = 1, uint32_t max_period = 0, uint32_t min_len = 0) const
    {
        const size_t n = text_.size();
        Runs r{std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
        const sfx_runs_filter_t flt{min_period, max_period, min_len, 0};
        uint64_t z = 0;
        if (n)
            check(sfx_runs_u32(bytes(text_), n, table_.data(), nullptr, &flt, r.begin.data(), r.end.data(), r.period.data(), n, &z), "runs");
        r.begin.resize((size_t)z);
        r.end.resize((size_t)z);
        r.period.resize((size_t)z);
        return r;
    }
    std::vector<uint32_t> lyndon_array(int order = 0) const
    {
        if (order != 0 && order != 1) throw std::invalid_argument("lyndon_array: order must be 0 or 1");
        std::vector<uint32_t> lyn(text_.size());
        if (!lyn.empty())
            check(sfx_lyndon_array_u32(bytes(text_), text_.size(), order == 0 ? table_.data() : nullptr, order, lyn.data()), "lyndon_array");
        return lyn;
    }
    std::vector<uint32_t> lyndon_factorization() const
    {
        const std::vector<uint32_t> lyn = lyndon_array(0);
        std::vector<uint32_t> starts;
        for (size_t i = 0; i < lyn.size(); i += lyn[i]) starts.push_back((uint32_t)i);
        return starts;
    }

private:
    SuffixTable() = default;
    static const uint8_t* bytes(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }
    static void check(int status, const char* what)
    {
        if (status == SFX_OK) return;
        std::string msg = std::string(what) + ": " + sfx_strerror(status) + " " + sfx_last_hip_error();
        if (status == SFX_ERR_TOO_LARGE) throw std::length_error(msg);               // assert! at :380
        throw std::runtime_error(msg);
    }
    // The device-resident index is made on the first query.  positions(&self) is lock-free and callable
    // from many threads in the reference, so the lazy creation must be race-free: std::call_once; a
    // creation that throws leaves the flag unset and the next caller tries again.  Queries on the finished
    // index only read it (the C ABI's *_batch calls are safe to run concurrently on one sfx_index).
    struct LazyIndex {
        std::once_flag once;
        sfx_index* ix = nullptr;
        std::once_flag lce_once;
        sfx_lce* lx = nullptr;
        ~LazyIndex() { if (ix) sfx_index_destroy(ix); if (lx) sfx_lce_destroy(lx); }
    };
    sfx_index* index() const
    {
        LazyIndex& l = *lazy_;
        std::call_once(l.once, [&] {
            check(sfx_index_create(bytes(text_), text_.size(), table_.data(), &l.ix), "sfx_index_create");
        });
        return l.ix;
    }
    sfx_lce* lce_index() const
    {
        LazyIndex& l = *lazy_;
        std::call_once(l.lce_once, [&] {
            const std::vector<uint32_t> lcp = lcp_lens();
            check(sfx_lce_create(table_.data(), lcp.data(), table_.size(), nullptr, 0, &l.lx), "sfx_lce_create");
        });
        return l.lx;
    }
    std::string text_;
    std::vector<uint32_t> table_;
    mutable std::unique_ptr<LazyIndex> lazy_ = std::make_unique<LazyIndex>();
};

inline std::string unlz(const std::vector<uint32_t>& len, const std::vector<uint32_t>& src, std::string_view lit)
{
    return SuffixTable::unlz(len, src, lit);
}

// additive: backward search over the pair of SuffixTable::bwt (suffix_hip.h, sfx_fm_*): count / contains / positions of a
// pattern from (bwt, samples) alone.  The handle lives in device memory (about 1.4 n bytes: nbytes()); neither the text
// nor the table is kept.  positions(q) equals SuffixTable::positions(q) element for element, in table order.
class FmIndex {
public:
    static FmIndex from_bwt(std::string_view bwt, const std::vector<uint32_t>& samples, uint32_t sample_step, uint32_t occ_step = 0)
    {
        FmIndex fm;
        check(sfx_fm_create(reinterpret_cast<const uint8_t*>(bwt.data()), bwt.size(), samples.data(), samples.size(), sample_step,
                            occ_step, &fm.h_), "FmIndex::from_bwt");
        check(sfx_fm_info(fm.h_, &fm.info_), "sfx_fm_info");
        return fm;
    }
    static FmIndex from_table(const SuffixTable& st, uint32_t sample_step = 64, uint32_t occ_step = 0)
    {
        const SuffixTable::Bwt tr = st.bwt(sample_step);
        return from_bwt(tr.bwt, tr.samples, sample_step, occ_step);
    }
    static FmIndex from_text(std::string text, uint32_t sample_step = 64, uint32_t occ_step = 0)
    {
        return from_table(SuffixTable::new_(std::move(text)), sample_step, occ_step);
    }
    FmIndex(FmIndex&& o) noexcept : h_(o.h_), info_(o.info_) { o.h_ = nullptr; }
    FmIndex& operator=(FmIndex&& o) noexcept
    {
        if (this != &o) { if (h_) sfx_fm_destroy(h_); h_ = o.h_; info_ = o.info_; o.h_ = nullptr; }
        return *this;
    }
    FmIndex(const FmIndex&) = delete;
    FmIndex& operator=(const FmIndex&) = delete;
    ~FmIndex() { if (h_) sfx_fm_destroy(h_); }

    size_t len() const { return (size_t)info_.n; }
    uint64_t nbytes() const { return info_.bytes; }
    const sfx_fm_info_t& info() const { return info_; }
    // (start, end) table ranks per pattern, (0, 0) where there is no match: what SuffixTable::positions_batch returns
    std::vector<std::pair<uint32_t, uint32_t>> count_batch(const std::vector<std::string_view>& qs) const
    {
        std::vector<uint64_t> off(qs.size() + 1, 0);
        std::string blob;
        for (size_t k = 0; k < qs.size(); k++) { blob.append(qs[k]); off[k + 1] = blob.size(); }
        std::vector<uint32_t> s(qs.size()), e(qs.size());
        if (!qs.empty())
            check(sfx_fm_count(h_, reinterpret_cast<const uint8_t*>(blob.data()), off.data(), qs.size(), s.data(), e.data()), "FmIndex::count");
        std::vector<std::pair<uint32_t, uint32_t>> out(qs.size());
        for (size_t k = 0; k < qs.size(); k++) out[k] = {s[k], e[k]};
        return out;
    }
    uint64_t count(std::string_view q) const { const auto se = count_batch({q}); return se[0].second - se[0].first; }
    bool contains(std::string_view q) const { return count(q) > 0; }
    // table entries of the ranks first .. first + count - 1 (UINT32_MAX for a rank >= len())
    std::vector<uint32_t> sa_range(uint64_t first, uint64_t count) const
    {
        std::vector<uint32_t> pos((size_t)count);
        if (count) check(sfx_fm_lookup(h_, nullptr, first, count, pos.data()), "FmIndex::sa_range");
        return pos;
    }
    std::vector<uint32_t> lookup(const std::vector<uint32_t>& ranks) const
    {
        std::vector<uint32_t> pos(ranks.size());
        if (!ranks.empty()) check(sfx_fm_lookup(h_, ranks.data(), 0, ranks.size(), pos.data()), "FmIndex::lookup");
        return pos;
    }
    std::vector<uint32_t> positions(std::string_view q) const
    {
        const auto se = count_batch({q});
        return sa_range(se[0].first, se[0].second - se[0].first);
    }

private:
    FmIndex() = default;
    static void check(int status, const char* what)
    {
        if (status == SFX_OK) return;
        std::string msg = std::string(what) + ": " + sfx_strerror(status) + " " + sfx_last_hip_error();
        if (status == SFX_ERR_TOO_LARGE) throw std::length_error(msg);
        throw std::runtime_error(msg);
    }
    sfx_fm* h_ = nullptr;
    sfx_fm_info_t info_{};
};

}  // namespace suffix

// tools/suffix_array.cpp -- the `suffix-array <file>` driver of the reference
// (/root/reference/src/main.rs:8-15: read a file, SuffixTable::new, print "Suffixes: N"),
// over the MI355X engine's C++ host mirror (include/suffix_table.hpp -> libsuffix_hip.so),
// extended into the large-file driver SURVEY.md 8(f) asks for:
//
//   suffix-array FILE [--lcp] [--dump PREFIX] [--load PREFIX] [--query Q [--mismatches K]]... [--repeats L [--earlier]] [--lce I,J[,I,J...] [--mismatches K]] [--isa] [--match FILE2 [--min-len L | --mems L [--unique] [--max-pairs P]]] [--bwt PREFIX [--step S]] [--lz PREFIX [--min-len L]] [--runs [--min-period P] [--max-period Q] [--min-len L]] [--lyndon] [--time]
//
//   --dump PREFIX   write PREFIX.sa (and PREFIX.lcp with --lcp) as raw little-endian u32
//                   arrays -- the on-disk form SuffixTable::from_parts (:111-119) reloads
//   --load PREFIX   skip construction: from_parts(text, PREFIX.sa)
//   --query Q       positions(Q) (:223-259): prints count and the first few positions
//   --query Q --mismatches K
//                   (without --lce) the occurrences of Q with up to K <= 255 differing bytes (Hamming distance) instead of
//                   the exact ones: "approx_positions("Q", K): Z", then one "position<TAB>mismatches" line per occurrence,
//                   sorted by position
//   --repeats L     one "begin end" line per maximal run of bytes that lie inside a repeat of at least L bytes;
//                   with --earlier only repeats of something EARLIER in the file count (the first copy of everything
//                   stays out of the report: what a deduplication would keep)
//   --match FILE2   which parts of FILE2 already stand in FILE: "Shared with FILE2 (>= L bytes): K spans, B bytes", then
//                   one "begin end src" line per maximal run of FILE2's bytes inside a stretch of at least L bytes
//                   (--min-len L, default 32) that also occurs in FILE; src = a position in FILE of the match that
//                   starts at `begin`
//   --match FILE2 --mems L [--unique] [--max-pairs P]
//                   the maximal exact matches of at least L bytes between FILE2 and FILE instead of the spans: "MEMs with
//                   FILE2 (>= L bytes): Z matches, P pairs", then one "qpos tpos len" line per match -- FILE2[qpos .. qpos+len)
//                   == FILE[tpos .. tpos+len), extendable in neither direction -- ascending by qpos, then by the table rank
//                   of tpos; --unique keeps the matches whose bytes occur once in FILE; more than P candidate pairs
//                   (default 2^30) end with status 2 and a message naming the count
//   --lce I,J[,I,J...] [--mismatches K]
//                   one line "i j len" per pair: how far the suffixes at byte positions i and j agree when up to K bytes
//                   (default 0) may differ; 0 for a position equal to the file's length, 4294967295 for one above
//   --isa           the inverse table: "ISA: rank of the whole text R, of its last byte R"; with --dump also PREFIX.isa
//   --bwt PREFIX    write the Burrows-Wheeler transform: PREFIX.bwt (n raw bytes) and PREFIX.bwi (little-endian u32: the
//                   sample step S, then the sampled rows; --step S, 0 or a power of two, default 256)
//   suffix-array PREFIX.bwt --unbwt PREFIX.bwi --out OUT
//                   restore the file from such a pair (no table is built); a pair that is the transform of no file ends
//                   with status 2 and a message, and OUT is not written
//   suffix-array PREFIX.bwt --fm PREFIX.bwi --query Q... [--occ-step B]
//                   answer the queries from such a pair through an FM-index: the same positions("Q") lines as
//                   `suffix-array FILE --query Q`; no table is built and the text is never held (--occ-step B: the
//                   entries per occurrence block, a power of two in 32 .. 4096; default: chosen from the alphabet)
//   --lz PREFIX     write the greedy LZ77 factorization as PREFIX.lz and print "LZ77: z Z, literals K, longest L": a 16-byte
//                   header (the magic "SFXLZ1\0\0", u32 n, u32 z, little-endian), then len[z], src[z] (u32) and lit[z] (bytes);
//                   repeats shorter than --min-len L (default here: 1, the classical parse) become literals
//   suffix-array PREFIX.lz --unlz --out OUT
//                   restore the file from a factorization (no table is built); a truncated or corrupted one ends with
//                   status 2 and a message, and OUT is not written
//   --runs [--min-period P] [--max-period Q] [--min-len L]
//                   the maximal repetitions (tandem repeats) of FILE: "Runs: Z", then one "begin end period" line per run --
//                   FILE[begin .. end) has smallest period `period`, is at least two periods long and extends to neither
//                   side -- ascending by (begin, period); only periods in P .. Q and runs of at least L bytes (defaults: all)
//   --lyndon        the Lyndon factorization of FILE under byte order: "Lyndon factors: K", then one factor start per line
//   --time          wall-clock milliseconds of construction / LCP (host pointers, i.e.
//                   including the PCIe copies: the device-resident rate is bench.py's)
//
// Exit status: 0 ok, 1 usage / IO error, 2 engine error (message on stderr; the
// reference panics in those places, :380 / :117).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "suffix_table.hpp"

static bool read_file(const std::string& path, std::string* out)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    const std::streamsize n = f.tellg();
    f.seekg(0);
    out->resize((size_t)n);
    return n == 0 || (bool)f.read(&(*out)[0], n);
}
static bool write_u32(const std::string& path, const std::vector<uint32_t>& v)
{
    std::ofstream f(path, std::ios::binary);
    return f && (v.empty() || f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * 4)));
}
static bool read_u32(const std::string& path, std::vector<uint32_t>* v)
{
    std::string raw;
    if (!read_file(path, &raw) || raw.size() % 4) return false;
    v->resize(raw.size() / 4);
    if (!raw.empty()) memcpy(v->data(), raw.data(), raw.size());
    return true;
}
static const char kLzMagic[8] = {'S', 'F', 'X', 'L', 'Z', '1', 0, 0};
static double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv)
{
    std::string file, dump, load, match, bwt, unbwt, out, fm, lz;
    long long min_len = 32, step = 256, occ_step = 0, mems = -1, max_pairs = 1ll << 30;
    std::vector<std::string> queries;
    bool want_lcp = false, timing = false, earlier = false, unlz = false, min_len_given = false, unique = false, max_pairs_given = false;
    long long repeats = -1, mismatches = 0;
    bool want_isa = false, mismatches_given = false, want_runs = false, want_lyndon = false;
    long long min_period = 1, max_period = 0;
    std::vector<uint32_t> lce_pos;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto need = [&](const char* opt) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs an argument\n", opt); exit(1); }
            return argv[++i];
        };
        if (a == "--lcp") want_lcp = true;
        else if (a == "--time") timing = true;
        else if (a == "--dump") dump = need("--dump");
        else if (a == "--load") load = need("--load");
        else if (a == "--query") queries.push_back(need("--query"));
        else if (a == "--earlier") earlier = true;
        else if (a == "--match") match = need("--match");
        else if (a == "--min-len") {
            min_len = atoll(need("--min-len"));
            min_len_given = true;
            if (min_len < 1 || min_len > 0xFFFFFFFFll) { fprintf(stderr, "--min-len needs a length of at least 1\n"); return 1; }
        }
        else if (a == "--mems") {
            mems = atoll(need("--mems"));
            if (mems < 1 || mems > 0xFFFFFFFFll) { fprintf(stderr, "--mems needs a length of at least 1\n"); return 1; }
        }
        else if (a == "--unique") unique = true;
        else if (a == "--runs") want_runs = true;
        else if (a == "--lyndon") want_lyndon = true;
        else if (a == "--min-period" || a == "--max-period") {
            const long long v = atoll(need(a.c_str()));
            if (v < 1 || v > 0xFFFFFFFFll) { fprintf(stderr, "%s needs a period of at least 1\n", a.c_str()); return 1; }
            (a == "--min-period" ? min_period : max_period) = v;
        }
        else if (a == "--isa") want_isa = true;
        else if (a == "--lce") {
            // I,J[,I,J...]: an even number of positions
            const std::string v = need("--lce");
            size_t p = 0;
            while (p <= v.size()) {
                size_t e = v.find(',', p);
                if (e == std::string::npos) e = v.size();
                char* end = nullptr;
                const std::string tok = v.substr(p, e - p);
                const unsigned long long x = strtoull(tok.c_str(), &end, 10);
                if (tok.empty() || *end || tok[0] == '-' || x > 0xFFFFFFFFull) { fprintf(stderr, "--lce needs positions I,J[,I,J...]\n"); return 1; }
                lce_pos.push_back((uint32_t)x);
                p = e + 1;
            }
            if (lce_pos.size() % 2) { fprintf(stderr, "--lce needs an even number of positions\n"); return 1; }
        }
        else if (a == "--mismatches") {
            mismatches = atoll(need("--mismatches"));
            mismatches_given = true;
            if (mismatches < 0 || mismatches > 0xFFFFFFFFll) { fprintf(stderr, "--mismatches needs a count of at least 0\n"); return 1; }
        }
        else if (a == "--max-pairs") {
            max_pairs = atoll(need("--max-pairs"));
            max_pairs_given = true;
            if (max_pairs < 1) { fprintf(stderr, "--max-pairs needs a count of at least 1\n"); return 1; }
        }
        else if (a == "--bwt") bwt = need("--bwt");
        else if (a == "--unbwt") unbwt = need("--unbwt");
        else if (a == "--out") out = need("--out");
        else if (a == "--fm") fm = need("--fm");
        else if (a == "--lz") lz = need("--lz");
        else if (a == "--unlz") unlz = true;
        else if (a == "--occ-step") {
            occ_step = atoll(need("--occ-step"));
            if (occ_step < 32 || occ_step > 4096 || (occ_step & (occ_step - 1))) { fprintf(stderr, "--occ-step needs a power of two in 32 .. 4096\n"); return 1; }
        }
        else if (a == "--step") {
            step = atoll(need("--step"));
            if (step < 0 || step > 0x80000000ll || (step & (step - 1))) { fprintf(stderr, "--step needs 0 or a power of two\n"); return 1; }
        }
        else if (a == "--repeats") {
            repeats = atoll(need("--repeats"));
            if (repeats < 1 || repeats > 0xFFFFFFFFll) { fprintf(stderr, "--repeats needs a length of at least 1\n"); return 1; }
        }
        else if (!a.empty() && a[0] == '-') { fprintf(stderr, "unknown option %s\n", a.c_str()); return 1; }
        else file = a;
    }
    if (mems > 0 && match.empty()) { fprintf(stderr, "--mems needs --match FILE2\n"); return 1; }
    if (mismatches_given && lce_pos.empty() && queries.empty()) { fprintf(stderr, "--mismatches needs --lce I,J or --query Q\n"); return 1; }
    const bool approx = mismatches_given && lce_pos.empty();            // (with --lce the count belongs to it, and queries stay exact)
    if (approx && (mismatches > 255 || !fm.empty())) { fprintf(stderr, "--query Q --mismatches K needs K <= 255 and a text, not a transform (--fm)\n"); return 1; }
    if (mems > 0 && min_len_given && lz.empty()) { fprintf(stderr, "--mems L takes its length itself: --min-len belongs to the span report of --match alone\n"); return 1; }
    if (mems < 0 && (unique || max_pairs_given)) { fprintf(stderr, "--unique and --max-pairs need --mems L\n"); return 1; }
    if (!want_runs && (min_period != 1 || max_period != 0)) { fprintf(stderr, "--min-period and --max-period need --runs\n"); return 1; }
    if (file.empty()) {
        fprintf(stderr, "usage: suffix-array FILE [--lcp] [--dump PREFIX] [--load PREFIX] [--query Q [--mismatches K]]... [--repeats L [--earlier]] [--lce I,J[,I,J...] [--mismatches K]] [--isa] [--match FILE2 [--min-len L | --mems L [--unique] [--max-pairs P]]] [--bwt PREFIX [--step S]] [--lz PREFIX [--min-len L]] [--runs [--min-period P] [--max-period Q] [--min-len L]] [--lyndon] [--time]\n       suffix-array PREFIX.lz --unlz --out OUT\n       suffix-array PREFIX.bwt --fm PREFIX.bwi --query Q... [--occ-step B]\n");
        return 1;
    }
    std::string text;
    if (!read_file(file, &text)) { fprintf(stderr, "cannot read %s\n", file.c_str()); return 1; }
    if (!unbwt.empty()) {                                               // FILE is a transform: restore, build nothing
        if (out.empty()) { fprintf(stderr, "--unbwt needs --out OUT\n"); return 1; }
        std::vector<uint32_t> bwi;
        std::string raw;
        if (!read_file(unbwt, &raw)) { fprintf(stderr, "cannot read %s\n", unbwt.c_str()); return 1; }
        if (raw.size() % 4 || raw.size() < 4) { fprintf(stderr, "suffix-array: %s is no sample file (corrupted pair)\n", unbwt.c_str()); return 2; }
        bwi.resize(raw.size() / 4);
        memcpy(bwi.data(), raw.data(), raw.size());
        try {
            const uint32_t s = bwi[0];
            bwi.erase(bwi.begin());
            const std::string restored = suffix::SuffixTable::unbwt(text, bwi, s);
            std::ofstream f(out, std::ios::binary);
            if (!f || (!restored.empty() && !f.write(restored.data(), (std::streamsize)restored.size()))) {
                fprintf(stderr, "cannot write %s\n", out.c_str());
                return 1;
            }
            std::cout << "Restored: " << restored.size() << " bytes\n";
        } catch (const std::exception& ex) {
            fprintf(stderr, "suffix-array: %s and %s are no transform of any file (corrupted pair): %s\n", file.c_str(), unbwt.c_str(), ex.what());
            return 2;
        }
        return 0;
    }
    if (unlz) {                                                         // FILE is a factorization: restore, build nothing
        if (out.empty()) { fprintf(stderr, "--unlz needs --out OUT\n"); return 1; }
        uint32_t hdr[2] = {0, 0};
        if (text.size() >= 16) memcpy(hdr, text.data() + 8, 8);
        const uint64_t n = hdr[0], z = hdr[1];
        if (text.size() < 16 || memcmp(text.data(), kLzMagic, 8) != 0 || text.size() != 16 + 9 * z) {
            fprintf(stderr, "suffix-array: %s is no factorization (truncated or corrupted)\n", file.c_str());
            return 2;
        }
        std::vector<uint32_t> len((size_t)z), src((size_t)z);
        if (z) {
            memcpy(len.data(), text.data() + 16, 4 * z);
            memcpy(src.data(), text.data() + 16 + 4 * z, 4 * z);
        }
        try {
            const std::string restored = suffix::unlz(len, src, std::string_view(text.data() + 16 + 8 * z, (size_t)z));
            if (restored.size() != n) throw std::runtime_error("the lengths do not sum to the header's n");
            std::ofstream f(out, std::ios::binary);
            if (!f || (!restored.empty() && !f.write(restored.data(), (std::streamsize)restored.size()))) {
                fprintf(stderr, "cannot write %s\n", out.c_str());
                return 1;
            }
            std::cout << "Restored: " << restored.size() << " bytes\n";
        } catch (const std::exception& ex) {
            fprintf(stderr, "suffix-array: %s is no factorization of any file (corrupted): %s\n", file.c_str(), ex.what());
            return 2;
        }
        return 0;
    }
    if (!fm.empty()) {                                                  // FILE is a transform: query it, build nothing
        std::string raw;
        if (!read_file(fm, &raw)) { fprintf(stderr, "cannot read %s\n", fm.c_str()); return 1; }
        if (raw.size() % 4 || raw.size() < 4) { fprintf(stderr, "suffix-array: %s is no sample file (corrupted pair)\n", fm.c_str()); return 2; }
        std::vector<uint32_t> bwi(raw.size() / 4);
        memcpy(bwi.data(), raw.data(), raw.size());
        try {
            const uint32_t s = bwi[0];
            bwi.erase(bwi.begin());
            auto t0 = std::chrono::steady_clock::now();
            const suffix::FmIndex ix = suffix::FmIndex::from_bwt(text, bwi, s, (uint32_t)occ_step);
            std::string().swap(text);                                   // the index owns a copy in device memory
            std::cout << "Suffixes: " << ix.len() << "\n";
            if (timing) std::cout << "fm-index ms: " << ms_since(t0) << " (" << ix.nbytes() << " bytes)\n";
            std::vector<std::string_view> qs(queries.begin(), queries.end());
            const auto se = ix.count_batch(qs);
            for (size_t k = 0; k < qs.size(); k++) {
                const uint32_t st = se[k].first, e = se[k].second;
                const std::vector<uint32_t> pos = ix.sa_range(st, std::min<uint32_t>(e - st, 8));
                std::cout << "positions(\"" << queries[k] << "\"): " << (e - st);
                for (size_t r = 0; r < pos.size(); r++) std::cout << (r == 0 ? " [" : ", ") << pos[r];
                if (e > st) std::cout << (e - st > 8 ? ", ...]" : "]");
                std::cout << "\n";
            }
        } catch (const std::exception& ex) {
            fprintf(stderr, "suffix-array: %s\n", ex.what());
            return 2;
        }
        return 0;
    }
    std::string other;
    if (!match.empty() && !read_file(match, &other)) { fprintf(stderr, "cannot read %s\n", match.c_str()); return 1; }
    try {
        auto t0 = std::chrono::steady_clock::now();
        suffix::SuffixTable st = [&] {
            if (load.empty()) return suffix::SuffixTable::new_(std::move(text));
            std::vector<uint32_t> sa;
            if (!read_u32(load + ".sa", &sa)) { fprintf(stderr, "cannot read %s.sa\n", load.c_str()); exit(1); }
            return suffix::SuffixTable::from_parts(std::move(text), std::move(sa));     // :111-119
        }();
        const double t_sa = ms_since(t0);
        std::cout << "Suffixes: " << st.len() << "\n";                                      // src/main.rs:14
        if (timing) std::cout << (load.empty() ? "construction" : "load") << " ms: " << t_sa << "\n";
        std::vector<uint32_t> lcp;
        if (want_lcp) {
            t0 = std::chrono::steady_clock::now();
            lcp = st.lcp_lens();
            if (timing) std::cout << "lcp ms: " << ms_since(t0) << "\n";
            uint64_t sum = 0;
            uint32_t mx = 0;
            for (uint32_t v : lcp) { sum += v; if (v > mx) mx = v; }
            std::cout << "LCP: max " << mx << " mean " << (lcp.empty() ? 0.0 : (double)sum / (double)lcp.size()) << "\n";
        }
        std::vector<uint32_t> isa;
        if (want_isa) {
            t0 = std::chrono::steady_clock::now();
            isa = st.inverse_table();
            if (timing) std::cout << "isa ms: " << ms_since(t0) << "\n";
            std::cout << "ISA: rank of the whole text " << (isa.empty() ? 0u : isa[0]) << ", of its last byte " << (isa.empty() ? 0u : isa.back()) << "\n";
        }
        if (!dump.empty()) {
            if (!write_u32(dump + ".sa", st.table()) || (want_lcp && !write_u32(dump + ".lcp", lcp)) || (want_isa && !write_u32(dump + ".isa", isa))) {
                fprintf(stderr, "cannot write %s.*\n", dump.c_str());
                return 1;
            }
        }
        if (approx) {
            for (const std::string& q : queries) {
                t0 = std::chrono::steady_clock::now();
                const auto occ = st.approx_positions(q, (uint32_t)mismatches);
                if (timing) std::cout << "approx ms: " << ms_since(t0) << "\n";
                std::cout << "approx_positions(\"" << q << "\", " << mismatches << "): " << occ.size() << "\n";
                for (const auto& pm : occ) std::cout << pm.first << "\t" << (unsigned)pm.second << "\n";
            }
        } else if (!queries.empty()) {
            std::vector<std::string_view> qs(queries.begin(), queries.end());
            auto se = st.positions_batch(qs);
            for (size_t k = 0; k < qs.size(); k++) {
                const uint32_t s = se[k].first, e = se[k].second;
                std::cout << "positions(\"" << queries[k] << "\"): " << (e - s);
                for (uint32_t r = s; r < e && r < s + 8; r++) std::cout << (r == s ? " [" : ", ") << st.table()[r];
                if (e > s) std::cout << (e - s > 8 ? ", ...]" : "]");
                std::cout << "\n";
            }
        }
        if (!lce_pos.empty()) {
            std::vector<uint32_t> a, b;
            for (size_t k = 0; k < lce_pos.size(); k += 2) { a.push_back(lce_pos[k]); b.push_back(lce_pos[k + 1]); }
            t0 = std::chrono::steady_clock::now();
            const auto len = st.lce_batch(a, b, (uint32_t)mismatches);
            if (timing) std::cout << "lce ms: " << ms_since(t0) << "\n";
            for (size_t k = 0; k < len.size(); k++) std::cout << a[k] << " " << b[k] << " " << len[k] << "\n";
        }
        if (repeats > 0) {
            t0 = std::chrono::steady_clock::now();
            const auto spans = st.repeated_spans((uint32_t)repeats, earlier ? SFX_REP_EARLIER : SFX_REP_ANY);
            if (timing) std::cout << "repeats ms: " << ms_since(t0) << "\n";
            for (const auto& be : spans) std::cout << be.first << " " << be.second << "\n";
        }
        if (!match.empty() && mems > 0) {
            t0 = std::chrono::steady_clock::now();
            const auto r = st.mems(other, (uint32_t)mems, unique, (uint64_t)max_pairs);
            if (timing) std::cout << "mems ms: " << ms_since(t0) << "\n";
            std::cout << "MEMs with " << match << " (>= " << mems << " bytes" << (unique ? ", unique" : "") << "): " << r.size() << " matches, "
                      << r.pairs << " pairs\n";
            for (size_t k = 0; k < r.size(); k++) std::cout << r.qpos[k] << " " << r.tpos[k] << " " << r.len[k] << "\n";
        } else if (!match.empty()) {
            t0 = std::chrono::steady_clock::now();
            const auto ms = st.match_stats(other, (uint32_t)min_len);           // a span report at L needs no more than max_len = L
            const auto spans = suffix::SuffixTable::spans_of(ms.len, (uint32_t)min_len);
            if (timing) std::cout << "match ms: " << ms_since(t0) << "\n";
            uint64_t covered = 0;
            for (const auto& be : spans) covered += be.second - be.first;
            std::cout << "Shared with " << match << " (>= " << min_len << " bytes): " << spans.size() << " spans, " << covered << " bytes\n";
            for (const auto& be : spans) std::cout << be.first << " " << be.second << " " << ms.src[be.first] << "\n";
        }
        if (want_runs) {
            t0 = std::chrono::steady_clock::now();
            const auto r = st.runs((uint32_t)min_period, (uint32_t)max_period, min_len_given ? (uint32_t)min_len : 0u);
            if (timing) std::cout << "runs ms: " << ms_since(t0) << "\n";
            std::cout << "Runs: " << r.size() << "\n";
            for (size_t k = 0; k < r.size(); k++) std::cout << r.begin[k] << " " << r.end[k] << " " << r.period[k] << "\n";
        }
        if (want_lyndon) {
            t0 = std::chrono::steady_clock::now();
            const auto starts = st.lyndon_factorization();
            if (timing) std::cout << "lyndon ms: " << ms_since(t0) << "\n";
            std::cout << "Lyndon factors: " << starts.size() << "\n";
            for (uint32_t b : starts) std::cout << b << "\n";
        }
        if (!bwt.empty()) {
            t0 = std::chrono::steady_clock::now();
            const auto tr = st.bwt((uint32_t)step);
            if (timing) std::cout << "bwt ms: " << ms_since(t0) << "\n";
            std::vector<uint32_t> bwi(1, (uint32_t)step);
            bwi.insert(bwi.end(), tr.samples.begin(), tr.samples.end());
            std::ofstream f(bwt + ".bwt", std::ios::binary);
            if (!f || (!tr.bwt.empty() && !f.write(tr.bwt.data(), (std::streamsize)tr.bwt.size())) || !write_u32(bwt + ".bwi", bwi)) {
                fprintf(stderr, "cannot write %s.*\n", bwt.c_str());
                return 1;
            }
            std::cout << "BWT: primary " << (tr.samples.empty() ? 0u : tr.samples[0]) << ", " << tr.samples.size() << " samples (step " << step
                      << ")\n";
        }
        if (!lz.empty()) {
            t0 = std::chrono::steady_clock::now();
            const auto f = st.lz77(min_len_given ? (uint32_t)min_len : 1u);
            if (timing) std::cout << "lz77 ms: " << ms_since(t0) << "\n";
            uint64_t literals = 0;
            uint32_t longest = 0;
            for (size_t k = 0; k < f.size(); k++) {
                literals += f.src[k] == 0xFFFFFFFFu;
                if (f.len[k] > longest) longest = f.len[k];
            }
            const uint32_t hdr[2] = {(uint32_t)st.len(), (uint32_t)f.size()};
            std::ofstream o(lz + ".lz", std::ios::binary);
            if (!o || !o.write(kLzMagic, 8) || !o.write(reinterpret_cast<const char*>(hdr), 8)
                || (f.size() && (!o.write(reinterpret_cast<const char*>(f.len.data()), (std::streamsize)(4 * f.size()))
                                 || !o.write(reinterpret_cast<const char*>(f.src.data()), (std::streamsize)(4 * f.size()))
                                 || !o.write(f.lit.data(), (std::streamsize)f.size())))) {
                fprintf(stderr, "cannot write %s.lz\n", lz.c_str());
                return 1;
            }
            std::cout << "LZ77: z " << f.size() << ", literals " << literals << ", longest " << longest << "\n";
        }
    } catch (const std::exception& ex) {
        fprintf(stderr, "suffix-array: %s\n", ex.what());
        return 2;
    }
    return 0;
}

// The C++ host mirror's both-strand search: complement_ranks at compile time, search_both_strands (batch, status-out and
// single-query forms, natural and explicit table, Hamming and edit) against search_approx / search_edit of the query and of
// its host-made reverse complement.  Compiled with the flags of tests/test_host_cpp.py and run on the GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <kmer_index_amd/kmer_index.hpp>

using kmer::alphabet::dna4;
using kmer::alphabet::dna5;
using kmer::alphabet::dna15;

// the tables, derived from the character tables at compile time
static_assert(kmer::alphabet::complement_ranks<dna4>() == std::array<std::uint8_t, 4>{3, 2, 1, 0});
static_assert(kmer::alphabet::complement_ranks<dna5>() == std::array<std::uint8_t, 5>{4, 2, 1, 3, 0});      // ACGNT: N to N
static_assert(kmer::alphabet::complement_char('R') == 'Y' && kmer::alphabet::complement_char('B') == 'V' &&
              kmer::alphabet::complement_char('D') == 'H' && kmer::alphabet::complement_char('K') == 'M' &&
              kmer::alphabet::complement_char('S') == 'S' && kmer::alphabet::complement_char('W') == 'W');
static constexpr bool dna15_is_iupac()
{
    constexpr auto t = kmer::alphabet::complement_ranks<dna15>();
    for (std::size_t r = 0; r < 15; ++r)
        if (kmer::alphabet::dna15_chars[t[r]] != kmer::alphabet::complement_char(kmer::alphabet::dna15_chars[r]) || t[t[r]] != r) return false;
    return true;
}
static_assert(dna15_is_iupac());

static std::uint64_t mix64(std::uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("CHECK failed: %s (line %d)\n", #cond, __LINE__); ++failures; } } while (0)

template<typename table_t>
static std::vector<dna4> revcomp(const std::vector<dna4>& q, const table_t& comp)
{
    std::vector<dna4> out(q.size());
    for (std::size_t i = 0; i < q.size(); ++i) out[i].assign_rank(comp[q[q.size() - 1 - i].to_rank()]);
    return out;
}

struct merged
{
    std::vector<std::uint32_t> positions, lengths;
    std::vector<std::uint8_t> distances, strands;
};

// two hit lists, each ascending, by (position, strand)
static merged merge(const std::vector<std::uint32_t>& fp, const std::vector<std::uint8_t>& fd, const std::vector<std::uint32_t>& fl,
                    const std::vector<std::uint32_t>& rp, const std::vector<std::uint8_t>& rd, const std::vector<std::uint32_t>& rl)
{
    merged m;
    std::size_t a = 0, b = 0;
    while (a < fp.size() || b < rp.size())
    {
        const bool fwd = b == rp.size() || (a < fp.size() && fp[a] <= rp[b]);
        m.positions.push_back(fwd ? fp[a] : rp[b]);
        m.distances.push_back(fwd ? fd[a] : rd[b]);
        if (!fl.empty() || !rl.empty()) m.lengths.push_back(fwd ? fl[a] : rl[b]);
        m.strands.push_back(fwd ? 0 : 1);
        fwd ? ++a : ++b;
    }
    return m;
}

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    const std::size_t n = 3000;
    std::vector<dna4> text(n);
    for (std::size_t i = 0; i < n; ++i) text[i].assign_rank(std::uint8_t(((mix64(i + 1) >> 32) * 4) >> 32));
    constexpr auto natural = kmer::alphabet::complement_ranks<dna4>();
    // a 16-letter window that is its own reverse complement, planted at offset 500: every hit of it comes on both strands
    std::vector<dna4> self_rc(text.begin() + 500, text.begin() + 508);
    {
        const std::vector<dna4> back = revcomp(self_rc, natural);
        self_rc.insert(self_rc.end(), back.begin(), back.end());
        std::copy(self_rc.begin(), self_rc.end(), text.begin() + 500);
    }
    auto index = kmer::make_kmer_index<8, 10, 12>(text, 4);
    using index_t = decltype(index);
    std::printf("index built\n");
    const index_t::complement_table swap_ac{1, 0, 2, 3};            // an involution that is not the complement

    std::size_t reverse_hits = 0, both = 0;
    for (std::size_t e = 0; e <= KMX_APPROX_MAX_SUBST; ++e)
    {
        std::vector<std::vector<dna4>> queries;
        for (std::size_t t = 0; t < 12; ++t)
        {
            const std::size_t m = 12 + (t * 7) % 30;
            const std::size_t s = t == 0 ? 0 : t == 1 ? n - m : mix64(1000 + t + 97 * e) % (n - m + 1);
            std::vector<dna4> q(text.begin() + s, text.begin() + s + m);
            for (std::size_t d = 0; d < (t % (e + 1)); ++d)
            {
                const std::size_t c = mix64(5000 + t * 13 + d) % q.size();
                q[c].assign_rank(std::uint8_t((q[c].to_rank() + 1 + d) % 4));
            }
            if (t % 2) q = revcomp(q, natural);
            queries.push_back(std::move(q));
        }
        queries.push_back(self_rc);
        std::vector<std::vector<dna4>> rc;
        for (auto const& q : queries) rc.push_back(revcomp(q, natural));

        for (int edit = 0; edit < 2; ++edit)
        {
            const auto hits = index.search_both_strands(queries, e, edit != 0);
            std::printf("e = %zu, edit = %d: searched\n", e, edit);
            CHECK(hits.size() == queries.size());
            for (std::size_t i = 0; i < queries.size(); ++i)
            {
                merged want;
                if (edit)
                {
                    const auto f = index.search_edit(queries[i], e), r = index.search_edit(rc[i], e);
                    want = merge(f.positions, f.distances, f.lengths, r.positions, r.distances, r.lengths);
                }
                else
                {
                    const auto f = index.search_approx(queries[i], e), r = index.search_approx(rc[i], e);
                    want = merge(f.positions, f.mismatches, {}, r.positions, r.mismatches, {});
                }
                CHECK(hits[i].positions == want.positions);
                CHECK(hits[i].distances == want.distances);
                CHECK(hits[i].strands == want.strands);
                CHECK(hits[i].lengths == want.lengths);
                CHECK(!hits[i].positions.empty());
                for (std::size_t h = 0; h < want.strands.size(); ++h) reverse_hits += want.strands[h];
                for (std::size_t h = 1; h < want.positions.size(); ++h) both += want.positions[h] == want.positions[h - 1];
            }
            // the single-query, status-out and explicit-table forms
            const auto one = index.search_both_strands(queries[3], e, edit != 0);
            CHECK(one.positions == hits[3].positions && one.strands == hits[3].strands && one.lengths == hits[3].lengths);
            std::vector<std::uint8_t> status;
            const auto with_status = index.search_both_strands(queries, e, edit != 0, status);
            CHECK(status == std::vector<std::uint8_t>(queries.size(), KMX_Q_OK));
            CHECK(with_status[5].positions == hits[5].positions && with_status[5].strands == hits[5].strands);
            const auto explicit_table = index.search_both_strands(queries, e, edit != 0, natural);
            CHECK(explicit_table[7].positions == hits[7].positions && explicit_table[7].strands == hits[7].strands);
            const auto other = index.search_both_strands(queries[3], e, edit != 0, swap_ac);   // query 3 is a reverse-strand read
            CHECK(std::count(other.strands.begin(), other.strands.end(), 1) < std::count(one.strands.begin(), one.strands.end(), 1));
        }
    }
    CHECK(reverse_hits > 0 && both > 0);
    const std::vector<std::vector<dna4>> first40{std::vector<dna4>(text.begin(), text.begin() + 40)};
    CHECK(index.search_both_strands(first40, 1).front().lengths.empty());              // edit defaults to false: no lengths
    CHECK(index.search_both_strands(first40, 1, true).front().lengths.size() == index.search_both_strands(first40, 1, true).front().positions.size());

    bool threw = false;
    try { (void)index.search_both_strands(std::vector<std::vector<dna4>>{first40.front(), std::vector<dna4>(2)}, 3); }
    catch (const index_t::approx_query_error& ex) { threw = ex.query_index == 1 && ex.status[1] == KMX_Q_TOO_SHORT && ex.status[0] == KMX_Q_OK; }
    CHECK(threw);
    threw = false;
    try { (void)index.search_both_strands(first40, 1, false, index_t::complement_table{1, 2, 0, 3}); }
    catch (const std::exception&) { threw = true; }               // not an involution: refused by the engine
    CHECK(threw);

    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("strands api ok\n");
    return 0;
}

// The C++ host mirror's reporting overloads (report_options on search_approx, search_edit and search_both_strands) against
// the three rules of kmx.h applied by plain loops to the exhaustive lists of the overloads without options.  Compiled with
// the flags of tests/test_host_cpp.py and run on the GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>

#include <kmer_index_amd/kmer_index.hpp>

using kmer::alphabet::dna4;

static std::uint64_t mix64(std::uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("CHECK failed: %s (line %d)\n", #cond, __LINE__); ++failures; } } while (0)

struct hit
{
    std::uint32_t p; std::uint8_t strand, d; std::uint32_t len;
    bool operator==(const hit&) const = default;
};

// the three steps of the contract, as it states them
static std::vector<hit> report(std::vector<hit> h, std::size_t e, bool loci, bool best, std::size_t max_hits, std::size_t& found)
{
    if (loci)
    {
        std::vector<hit> kept;
        for (auto const& x : h)
        {
            bool dead = false;
            for (auto const& y : h)
            {
                const std::uint32_t gap = x.p > y.p ? x.p - y.p : y.p - x.p;
                if (y.strand == x.strand && y.p != x.p && gap <= e && std::make_pair(y.d, y.p) < std::make_pair(x.d, x.p)) dead = true;
            }
            if (!dead) kept.push_back(x);
        }
        h = kept;
    }
    if (best && !h.empty())
    {
        std::uint8_t least = 255;
        for (auto const& x : h) least = std::min(least, x.d);
        std::erase_if(h, [&](const hit& x) { return x.d != least; });
    }
    found = h.size();
    if (max_hits && h.size() > max_hits)
    {
        std::sort(h.begin(), h.end(), [](const hit& a, const hit& b) { return std::make_tuple(a.d, a.p, a.strand) < std::make_tuple(b.d, b.p, b.strand); });
        h.resize(max_hits);
        std::sort(h.begin(), h.end(), [](const hit& a, const hit& b) { return std::make_pair(a.p, a.strand) < std::make_pair(b.p, b.strand); });
    }
    return h;
}

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    // 300 random letters, 12 copies of a 100-letter unit with three letters of each substituted, 300 random letters
    std::vector<dna4> text;
    auto letter = [](std::uint64_t i) { dna4 l; l.assign_rank(std::uint8_t(((mix64(i + 1) >> 32) * 4) >> 32)); return l; };
    for (std::size_t i = 0; i < 300; ++i) text.push_back(letter(i));
    for (std::size_t c = 0; c < 12; ++c)
        for (std::size_t i = 0; i < 100; ++i)
        {
            dna4 l = letter(10000 + i);
            if (mix64(77 * c + i) % 33 == 0) l.assign_rank(std::uint8_t((l.to_rank() + 1 + c % 3) % 4));
            text.push_back(l);
        }
    for (std::size_t i = 0; i < 300; ++i) text.push_back(letter(20000 + i));
    const std::size_t n = text.size();
    auto index = kmer::make_kmer_index<5>(text, 4);
    using index_t = decltype(index);
    std::printf("index built\n");

    std::vector<std::vector<dna4>> queries;
    for (std::size_t t = 0; t < 16; ++t)
    {
        const std::size_t m = 22 + t % 5, s = 250 + mix64(300 + t) % (n - 500);
        std::vector<dna4> q(text.begin() + s, text.begin() + s + m);
        if (t % 3 == 1) q[m / 2].assign_rank(std::uint8_t((q[m / 2].to_rank() + 1) % 4));
        if (t % 4 == 3)                                                            // a read of the other strand
        {
            std::vector<dna4> back(m);
            for (std::size_t i = 0; i < m; ++i) back[i].assign_rank(std::uint8_t(3 - q[m - 1 - i].to_rank()));
            q = back;
        }
        queries.push_back(std::move(q));
    }

    std::size_t by_loci = 0, by_best = 0, cut = 0, uncut = 0;
    std::vector<std::uint8_t> status;
    for (std::size_t e = 0; e <= KMX_APPROX_MAX_SUBST; ++e)
        for (int mode = 0; mode < 4; ++mode)                                       // Hamming, edit, both strands Hamming, both strands edit
        {
            const bool edit = mode & 1, strands = mode & 2;
            std::vector<std::vector<hit>> H(queries.size());
            if (strands)
            {
                const auto all = index.search_both_strands(queries, e, edit, status);
                for (std::size_t i = 0; i < all.size(); ++i)
                    for (std::size_t k = 0; k < all[i].positions.size(); ++k)
                        H[i].push_back({all[i].positions[k], all[i].strands[k], all[i].distances[k], edit ? all[i].lengths[k] : 0u});
            }
            else if (edit)
            {
                const auto all = index.search_edit(queries, e, status);
                for (std::size_t i = 0; i < all.size(); ++i)
                    for (std::size_t k = 0; k < all[i].positions.size(); ++k)
                        H[i].push_back({all[i].positions[k], 0, all[i].distances[k], all[i].lengths[k]});
            }
            else
            {
                const auto all = index.search_approx(queries, e, status);
                for (std::size_t i = 0; i < all.size(); ++i)
                    for (std::size_t k = 0; k < all[i].positions.size(); ++k) H[i].push_back({all[i].positions[k], 0, all[i].mismatches[k], 0u});
            }
            CHECK(status == std::vector<std::uint8_t>(queries.size(), KMX_Q_OK));
            for (int combo = 1; combo < 12; ++combo)
            {
                index_t::report_options opt;
                opt.loci = edit && (combo & 1);
                opt.best = combo & 2;
                opt.max_hits = combo < 4 ? 0 : combo < 8 ? 1 : 3;
                if (!opt.loci && !opt.best && !opt.max_hits) continue;
                std::vector<std::vector<hit>> got(queries.size());
                std::vector<std::size_t> found(queries.size());
                if (strands)
                {
                    const auto r = index.search_both_strands(queries, e, edit, opt, status);
                    for (std::size_t i = 0; i < r.size(); ++i)
                    {
                        found[i] = r[i].found;
                        CHECK(r[i].lengths.size() == (edit ? r[i].positions.size() : 0));
                        for (std::size_t k = 0; k < r[i].positions.size(); ++k)
                            got[i].push_back({r[i].positions[k], r[i].strands[k], r[i].distances[k], edit ? r[i].lengths[k] : 0u});
                    }
                }
                else if (edit)
                {
                    const auto r = index.search_edit(queries, e, opt, status);
                    for (std::size_t i = 0; i < r.size(); ++i)
                    {
                        found[i] = r[i].found;
                        for (std::size_t k = 0; k < r[i].positions.size(); ++k)
                            got[i].push_back({r[i].positions[k], 0, r[i].distances[k], r[i].lengths[k]});
                    }
                }
                else
                {
                    const auto r = index.search_approx(queries, e, opt, status);
                    for (std::size_t i = 0; i < r.size(); ++i)
                    {
                        found[i] = r[i].found;
                        for (std::size_t k = 0; k < r[i].positions.size(); ++k) got[i].push_back({r[i].positions[k], 0, r[i].mismatches[k], 0u});
                    }
                }
                CHECK(status == std::vector<std::uint8_t>(queries.size(), KMX_Q_OK));
                for (std::size_t i = 0; i < queries.size(); ++i)
                {
                    std::size_t want_found = 0, unused = 0;
                    const auto want = report(H[i], e, opt.loci, opt.best, opt.max_hits, want_found);
                    CHECK(got[i] == want);
                    CHECK(found[i] == want_found);
                    if (opt.loci && !opt.best && !opt.max_hits) by_loci += H[i].size() - want.size();
                    if (opt.best && !opt.loci && !opt.max_hits) by_best += H[i].size() - report(H[i], e, false, true, 0, unused).size();
                    if (opt.max_hits) (want_found > want.size() ? cut : uncut) += 1;
                }
            }
            std::printf("e = %zu, mode = %d: checked\n", e, mode);
        }
    CHECK(by_loci > 0 && by_best > 0 && cut > 0 && uncut > 0);

    // loci without edit is refused by the engine; the overloads without options leave found at 0
    bool threw = false;
    try { index_t::report_options opt; opt.loci = true; (void)index.search_approx(queries, 1, opt, status); }
    catch (const std::exception&) { threw = true; }
    CHECK(threw);
    CHECK(index.search_edit(queries, 1, status).front().found == 0);

    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("report api ok\n");
    return 0;
}

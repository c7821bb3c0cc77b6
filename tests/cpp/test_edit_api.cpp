// The C++ host mirror's edit-distance search: make_kmer_index<8, 10, 12> on a small text, search_edit against a brute-force
// loop over every start and window length.  Compiled with the flags of tests/test_host_cpp.py and run on the GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

// Levenshtein distance of q to text[p, p + len)
static std::size_t lev(const std::vector<dna4>& q, const std::vector<dna4>& text, std::size_t p, std::size_t len)
{
    std::vector<std::size_t> prev(len + 1), cur(len + 1);
    for (std::size_t c = 0; c <= len; ++c) prev[c] = c;
    for (std::size_t i = 1; i <= q.size(); ++i)
    {
        cur[0] = i;
        for (std::size_t c = 1; c <= len; ++c)
            cur[c] = std::min({prev[c - 1] + !(q[i - 1] == text[p + c - 1]), prev[c] + 1, cur[c - 1] + 1});
        std::swap(prev, cur);
    }
    return prev[len];
}

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    const std::size_t n = 3000;
    std::vector<dna4> text(n);
    for (std::size_t i = 0; i < n; ++i) text[i].assign_rank(std::uint8_t(((mix64(i + 1) >> 32) * 4) >> 32));
    auto index = kmer::make_kmer_index<8, 10, 12>(text, 4);
    std::printf("index built\n");

    std::size_t other_length = 0;
    for (std::size_t e = 0; e <= KMX_APPROX_MAX_SUBST; ++e)
    {
        std::vector<std::vector<dna4>> queries;
        for (std::size_t t = 0; t < 12; ++t)
        {
            const std::size_t m = 12 + (t * 7) % 30;
            const std::size_t s = t == 0 ? 0 : t == 1 ? n - m : mix64(1000 + t + 97 * e) % (n - m + 1);
            std::vector<dna4> q(text.begin() + s, text.begin() + s + m);
            for (std::size_t d = 0; d < (t % (e + 2)); ++d)
            {
                const std::size_t c = mix64(5000 + t * 13 + d) % q.size();
                const std::size_t kind = mix64(7000 + t * 5 + d + e) % 3;
                if (kind == 0) q[c].assign_rank(std::uint8_t((q[c].to_rank() + 1 + d) % 4));
                else if (kind == 1) q.erase(q.begin() + c);
                else q.insert(q.begin() + c, q[(c + 3) % q.size()]);
            }
            queries.push_back(std::move(q));
        }
        const auto hits = index.search_edit(queries, e);
        std::printf("e = %zu: searched\n", e);
        CHECK(hits.size() == queries.size());
        for (std::size_t i = 0; i < queries.size(); ++i)
        {
            const auto& q = queries[i];
            const std::size_t m = q.size();
            std::vector<std::uint32_t> want, want_len;
            std::vector<std::uint8_t> want_d;
            for (std::size_t p = 0; p < n; ++p)
            {
                std::size_t best_d = e + 1, best_len = 0;
                for (std::size_t len = m > e ? m - e : 1; len <= m + e && p + len <= n; ++len)
                {
                    const std::size_t d = lev(q, text, p, len);
                    const std::size_t off = len > m ? len - m : m - len, best_off = best_len > m ? best_len - m : m - best_len;
                    if (d < best_d || (d == best_d && d <= e && off < best_off)) { best_d = d; best_len = len; }
                }
                if (best_d <= e) { want.push_back(std::uint32_t(p)); want_d.push_back(std::uint8_t(best_d)); want_len.push_back(std::uint32_t(best_len)); }
            }
            CHECK(hits[i].positions == want);
            CHECK(hits[i].distances == want_d);
            CHECK(hits[i].lengths == want_len);
            for (std::size_t h = 0; h < want_len.size(); ++h) other_length += want_len[h] != m;
        }
        const auto one = index.search_edit(queries[3], e);
        CHECK(one.positions == hits[3].positions);
        CHECK(one.lengths == hits[3].lengths);
    }
    CHECK(other_length > 0);
    bool threw = false;
    try { (void)index.search_edit(std::vector<std::vector<dna4>>{std::vector<dna4>(2)}, 3); }
    catch (const decltype(index)::approx_query_error& ex) { threw = ex.query_index == 0 && ex.status[0] == KMX_Q_TOO_SHORT; }
    CHECK(threw);

    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("edit api ok\n");
    return 0;
}

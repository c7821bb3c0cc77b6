// What the approximate search (kmx_approx.hip) needs from an index (kmx_capi.hip owns struct kmx_index).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>

#include "kmx_types.h"

namespace kmx {

// The text of one replica packed at w bits per letter (w = 2, 4 or 8: a letter never straddles a word), derived from the
// index on first use (kmx_index_text / kmx_search_approx) and kept until kmx_index_free.  `ready` is set only by a
// derivation that succeeded: a failed one (out of memory) leaves nothing behind and the next call tries again.
struct PackedText {
    std::mutex mu;
    bool ready = false;
    uint64_t* d_words = nullptr;
    uint64_t n_words = 0;      // ceil(n * w / 64) + KMX_TEXT_PAD_WORDS
    uint32_t w = 0;
};
#define KMX_TEXT_PAD_WORDS 4   // a window read of two words past any offset stays inside the allocation

// The contig table of one replica (kmx_index_set_contigs): contig c is text[off[c], off[c + 1]).  d_off is NULL and nc 0 while the
// index has no table.  gen counts the successful kmx_index_set_contigs calls on the index (the same in every replica): the
// alignments record it, and the calls behind them refuse a handle that was made under another table.
struct ContigTable {
    uint64_t* d_off = nullptr;     // [nc + 1], on the replica's device
    uint64_t nc = 0;
    uint64_t gen = 0;
};

struct IndexAccess {
    int device;
    uint64_t n;
    uint32_t sigma;
    uint32_t range;
    bool broken;
    const KmxIndexDev* h;      // host copy of the replica's header (device pointers)
    PackedText* text;
    const uint64_t* ctg_off;   // the replica's contig table (device, [nc + 1]); nullptr without one
    uint64_t nc, ctg_gen;
};
IndexAccess index_access(const kmx_index* ix);                  // kmx_capi.hip
// kmx_capi.hip: the replica of ix that lives on `device`; false when there is none
bool index_access_on(const kmx_index* ix, int device, IndexAccess* out);
// kmx_approx.hip: derives the replica's packed text on first use (the index's device is current; synchronises s when it derives)
kmx_status ensure_text(const IndexAccess& A, hipStream_t s);
// kmx_approx.hip: the refusals of a complement table (kmx_search_approx_strands, kmx_reads_strands); comp[256] <- the table, the
// identity outside the alphabet
kmx_status check_complement(const std::string& who, const uint8_t* complement, uint32_t sigma, uint8_t* comp);
// kmx_capi.hip: the caller has synchronised the stream of r's last search (no device-wide wait when r is freed)
void result_quiesced(kmx_result* r);
void packed_text_release(PackedText* t);                        // kmx_approx.hip (the index's device is current)

} // namespace kmx

// Internal launchers of sigjson.hip: the hash arrays of signature JSON parsed on the device (sigload.hpp is the host side).
// The records the kernels exchange and the rules they apply are in sigjson_core.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "sigjson_core.hpp"

namespace smg {

struct SjPiece { uint64_t src, dst, n; };

// d_base: the text block, with SJ_TEXT_PAD readable bytes behind its last document (sj_parse_launch loads whole 16-byte lines)
hipError_t sj_spans_launch(const uint8_t* d_base, const SjDoc* d_docs, uint32_t n_docs, SjSpan* d_spans, uint32_t* d_doc_flags, hipStream_t stream);
hipError_t sj_parse_launch(const uint8_t* d_base, const SjParse* d_jobs, uint32_t n_jobs, uint64_t* d_values, SjParsed* d_results, uint64_t keep_max,
                           hipStream_t stream);
hipError_t sj_take_bytes_launch(const uint8_t* d_base, const SjPiece* d_pieces, uint32_t n, uint8_t* d_out, hipStream_t stream);
hipError_t sj_take_u64_launch(const uint64_t* d_values, const SjPiece* d_pieces, uint32_t n, uint64_t* d_out, hipStream_t stream);

// From what sj_spans_launch found to what sj_parse_launch is given: a document with the odd bit, or with an odd array, is not
// taken; of every other document each `mins` array becomes a job, the values of the jobs side by side in job order; what lies
// outside a taken document's arrays is cut into pieces (one in front of every array, one behind the last) for sj_take_bytes_launch.
struct SjDocPlan { size_t job0 = 0, rest0 = 0, rest1 = 0; uint64_t rest_off = 0; bool take = false; };
struct SjPlan {
    std::vector<SjParse> jobs;
    std::vector<SjPiece> rest;                                        // pieces of text outside the arrays
    std::vector<SjDocPlan> docs;
    uint64_t n_values = 0, rest_bytes = 0;
};
inline void sj_plan(const std::vector<SjDoc>& docs, const SjSpan* spans, const uint32_t* flags, SjPlan& out) {
    out.jobs.clear(); out.rest.clear();
    out.docs.assign(docs.size(), SjDocPlan());
    out.n_values = out.rest_bytes = 0;
    for (size_t d = 0; d < docs.size(); ++d) {
        const uint32_t ns = flags[d] & 0xffu;
        bool odd = (flags[d] & SJ_DOC_ODD) != 0;
        for (uint32_t s = 0; s < ns && !odd; ++s) odd = (spans[d * SJ_MAX_SPANS + s].flags & SJ_SPAN_ODD) != 0;
        if (odd) continue;
        SjDocPlan& pl = out.docs[d];
        pl.take = true;
        pl.job0 = out.jobs.size();
        pl.rest0 = out.rest.size();
        pl.rest_off = out.rest_bytes;
        uint64_t at = 0;
        for (uint32_t s = 0; s < ns; ++s) {
            const SjSpan& sp = spans[d * SJ_MAX_SPANS + s];
            out.rest.push_back(SjPiece{docs[d].off + at, out.rest_bytes, sp.begin - at});
            out.rest_bytes += sp.begin - at;
            at = sp.end;
            if (sp.kind == SJ_MINS) {
                out.jobs.push_back(SjParse{docs[d].off + sp.begin, sp.end - sp.begin, out.n_values, sp.n_values});
                out.n_values += sp.n_values;
            }
        }
        out.rest.push_back(SjPiece{docs[d].off + at, out.rest_bytes, docs[d].len - at});
        out.rest_bytes += docs[d].len - at;
        pl.rest1 = out.rest.size();
    }
}

}  // namespace smg

// The caller's trace as every layer below the C ABI sees it: which of the four forms it has, where its memory is, and what follows from
// that -- the one refusal rule of a trace argument, and what the upload needs of the prover's buffers.  Host code, no HIP headers: it
// is part of the GPU library and of the host-only sanitizer builds alike.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "airs.h"

namespace starkhip {

struct TraceLog;  // trace_log.h

enum class TraceForm { RowMajor, ColMajor, Recording, ColumnTable };

struct TraceInput {  // a view; owns nothing
    TraceForm form = TraceForm::RowMajor;
    bool on_device = false;       // dense forms only: the words are device memory
    bool unknown_layout = false;  // dense(): the C ABI's layout was neither 0 nor 1 (check() refuses it)
    size_t n_rows = 0, n_cols = 0;
    union {
        const uint64_t* words = nullptr;   // RowMajor [n_rows][n_cols], ColMajor [n_cols][n_rows]
        const TraceLog* log;               // Recording
        const uint64_t* const* columns;    // ColumnTable: n_cols pointers to n_rows host words each
    };

    // layout and on_device as the C ABI spells them (0 row-major, 1 column-major; 0 host, otherwise device)
    static TraceInput dense(const uint64_t* words, size_t n_rows, size_t n_cols, int layout, int on_device);
    static TraceInput recording(const void* log);  // a starkhip_trace_log_* handle: rows and columns are the log's; null stays null
    static TraceInput column_table(const uint64_t* const* columns, size_t n_rows, size_t n_cols);

    // STARKHIP_ERR_BAD_SHAPE for a trace argument that cannot be a trace of `air`: a null pointer, an unknown layout, a column count
    // that is not the AIR's, a null column, a recording without rows, device memory in a form that has none.  Rows and public inputs
    // are the proof's to judge (ProofShape::make, check_trace_shape).
    int check(const AirInfo& air) const;
    size_t at(size_t row, size_t col) const { return form == TraceForm::ColMajor ? col * n_rows + row : row * n_cols + col; }  // dense forms: a cell's index in `words`
    bool callers_columns() const { return form == TraceForm::ColMajor && on_device; }  // read where it is: nothing is uploaded
    // 64-bit words the upload stages at the start of the LDE buffer for a trace of C columns: a recording's words, offsets and late
    // zeros, or host rows on their way through the transpose
    size_t park_words(size_t C) const;
    void to_row_major(std::vector<uint64_t>& rows) const;  // host dense forms only: a copy of the trace as [n_rows][n_cols]
};

}  // namespace starkhip

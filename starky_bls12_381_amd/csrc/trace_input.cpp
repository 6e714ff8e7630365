#include "trace_input.h"

#include "trace_log.h"

namespace starkhip {

TraceInput TraceInput::dense(const uint64_t* words, size_t n_rows, size_t n_cols, int layout, int on_device) {
    TraceInput in{layout == 1 ? TraceForm::ColMajor : TraceForm::RowMajor, on_device != 0, layout != 0 && layout != 1, n_rows, n_cols};
    in.words = words;
    return in;
}

TraceInput TraceInput::recording(const void* log) {
    const TraceLog* l = (const TraceLog*)log;
    TraceInput in{TraceForm::Recording, false, false, l ? l->rows : 0, l ? l->cols : 0};
    in.log = l;
    return in;
}

TraceInput TraceInput::column_table(const uint64_t* const* columns, size_t n_rows, size_t n_cols) {
    TraceInput in{TraceForm::ColumnTable, false, false, n_rows, n_cols};
    in.columns = columns;
    return in;
}

int TraceInput::check(const AirInfo& air) const {
    const bool dense = form == TraceForm::RowMajor || form == TraceForm::ColMajor;
    const bool null = dense ? !words : form == TraceForm::Recording ? !log : !columns;
    if (null || unknown_layout || n_cols != air.cols || (on_device && !dense)) return STARKHIP_ERR_BAD_SHAPE;
    if (form == TraceForm::Recording && !n_rows) return STARKHIP_ERR_BAD_SHAPE;  // no generator ran while it was armed
    if (form == TraceForm::ColumnTable)  // (the table is known to be n_cols long only now that n_cols is right)
        for (size_t i = 0; i < n_cols; i++)
            if (!columns[i]) return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}

size_t TraceInput::park_words(size_t C) const {
    if (form == TraceForm::Recording) return (log->total_words() + log->total_records() + log->total_late_zeros() + 2 + 1) / 2;
    return form == TraceForm::RowMajor && !on_device ? C * n_rows : 0;
}

void TraceInput::to_row_major(std::vector<uint64_t>& rows) const {
    rows.resize(n_rows * n_cols);
    for (size_t r = 0; r < n_rows; r++)
        for (size_t c = 0; c < n_cols; c++) rows[r * n_cols + c] = words[at(r, c)];
}

}  // namespace starkhip

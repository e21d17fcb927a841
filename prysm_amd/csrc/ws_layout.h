// Layout of a 2-D transform's private intermediate, stated ONCE: the planner (capi_plan.hip) sizes the workspace from it, the runner
// (capi_run.hip) fills the kernels' parameter blocks from it, tools/emu_fft.cpp runs the loaders and storers on the CPU against it.
// Plain C++: nothing from HIP here, and not part of pm_internal.h, which the kernel units include.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pm {

// every buffer of a workspace starts on a 256 B boundary
inline size_t align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }

// The tiled intermediate of ONE field, W[plane][tile][row][c % TL]: the columns are cut into layout tiles of TL = tc << log_k columns
// (2^log_k column tiles of the column pass side by side), a layout tile holds its rows as TL contiguous elements each, and a folded
// transform keeps two such planes of M/2 rows (the even / odd bins of the column transform).
struct TiledLayout {
    int tc = 0;           // column tile width of the column pass (a power of two); 0: the intermediate is not tiled
    int log_k = 0;        // layout tile width TL = tc << log_k
    int ltl = 0;          // log2(TL)
    int64_t cols = 0;     // columns held: N, or N/2 on the half-spectrum routes
    int64_t rows = 0;     // rows per plane
    int planes = 1;       // 2 when folded

    // `rows` rows of `cols` columns, as two planes of rows / 2 when folded.  log_k shrinks until the layout tile divides the columns (the
    // last layout tile would otherwise be padding the row pass never writes)
    static TiledLayout make(int tc, int log_k, int64_t cols, int64_t rows, bool folded = false) {
        while (log_k > 0 && (cols % (int64_t(tc) << log_k)) != 0) --log_k;
        int ltl = 0;
        while ((int64_t(1) << ltl) < (int64_t(tc) << log_k)) ++ltl;
        return TiledLayout{tc, log_k, ltl, cols, folded ? rows / 2 : rows, folded ? 2 : 1};
    }
    int64_t tl() const { return int64_t(1) << ltl; }
    int64_t ntl() const { return (cols + tl() - 1) / tl(); }           // layout tiles
    int ntiles() const { return int((cols + tc - 1) / tc); }           // column tiles = workgroups' worth of the column pass
    int64_t plane() const { return ntl() * rows * tl(); }              // elements from one plane to the next
    int64_t elems() const { return planes * plane(); }                 // elements per field
    size_t bytes(size_t es) const { return size_t(elems()) * es; }     // ... in bytes, es per element
};

}  // namespace pm

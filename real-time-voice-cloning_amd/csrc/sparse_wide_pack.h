// Block-sparse image of the fatchord step matrices for wide row batches ("the
// wide form"): per slot of an XCD group, the live 1 x 4 blocks of the slot's output rows of every
// product set as float4 lists with their column-block indices. Host only, plain C++
// (sparse_wide_pack.cpp, built by g++ like plan.cpp): the packer, its fit rule and the
// densified reconstruction the CPU tests compare with the matrix.
//
// The reference's Pruner zeroes 1 x 4 column blocks (vocoder/pruner.py:60-88); its native backend
// skips them (CompMatrix::operator*, vocoder/libwavernn/runtimeracer_version/src/wavernn.cpp:
// 162-184). A slot owns the rows the dense wide kernel's slot owns (kernels_persist_wide.hip: units
// / classes [16 w, 16 w + 16) of every 512-row gate or layer matrix), so the exchange layout of
// wide_layout.h serves both.
#pragma once
#include <cstdint>
#include <vector>

#include "plan_consts.h"

namespace wrnn {
namespace wsp {

constexpr int kSlots = kPM;          // 32 slots per group
constexpr int kRows = 16;            // output rows of a slot per product set
constexpr int kCols = kPH;           // K of every product (the x / h parts of the step matrices)
constexpr int kColBlocks = kCols / 4;
// product sets of a slot, in list order: W_ih2[:, :512] r, z, n | W_hh1 r, z, n | fc1 | fc2 |
// fc3 rows 16 w .. | fc3 rows 512 + 16 w .. (1024 classes; else empty) | W_hh2 r, z, n
enum Set : int { S_IH2 = 0, S_HH1 = 3, S_FC1 = 6, S_FC2 = 7, S_FC3 = 8, S_FC3B = 9, S_HH2 = 10, kSets = 13 };

// ---- the LDS carve a slot's lists must fit (bytes of the CU's 160 KiB) -----------------------
// What a step reads and writes besides the lists keeps the first 80 KiB (kernels_persist_wide_sp.hip:
// row tables, bias, the P1 and noise rings, the gh sums, the two X stages of 16 x 516 floats);
// the lists take the rest: the (start, count) pair of every (set, row) list as two 16-bit words,
// the column-block index of each block (16 bits), then kCapF4 blocks of 16 bytes -- the order of
// the device image of a slot (slot_image), copied into LDS as it is.
constexpr int kStepBytes = 80 * 1024;
constexpr int kCapF4 = 4096;
constexpr int kTabBytes = kSets * kRows * 4;
constexpr int kColBytes = kCapF4 * 2;
constexpr int kListBytes = kCapF4 * 16;
constexpr int kImgWords = (kTabBytes + kColBytes + kListBytes) / 4;  // 32-bit words of a slot's image
static_assert(kStepBytes + kTabBytes + kColBytes + kListBytes <= 160 * 1024, "sparse-wide LDS carve exceeds the CU's 160 KiB");
static_assert(kCapF4 <= 65535 && kColBlocks <= 65535, "list starts, counts and column blocks are 16-bit words");
static_assert((kStepBytes + kTabBytes + kColBytes) % 16 == 0 && kImgWords % 4 == 0, "the float4 lists stay 16-byte aligned");

// A block is dead when its four words are +0.0 or -0.0 (an explicitly stored zero block; any other
// bit pattern -- a denormal, a NaN -- is kept: the dense kernels multiply it too).
bool dead4(const float* p);

// The lists of consecutive output rows: row r's live blocks are blocks[4 (start[r] + i)], at
// column block col[start[r] + i], i < count[r], by ascending column -- the one order every
// accumulator of the row adds them in.
struct Lists {
    std::vector<uint16_t> start, count;  // per row
    std::vector<float> blocks;           // 4 floats per live block
    std::vector<uint16_t> col;           // column block of each (columns 4 c .. 4 c + 3)
    int size() const { return (int)col.size(); }
};
// Appends the lists of rows [row0, row0 + nrows) of the row-major matrix W (`rows` rows of `ld`
// floats; the first `cols` columns, a multiple of 4) to L. Rows at or beyond `rows` are empty.
// False (L unchanged) when a list start or size would pass the 16-bit words.
bool append_rows(const float* W, int rows, int ld, int cols, int row0, int nrows, Lists& L);
// Row r of L written back densely: out[0 .. cols) (zero-filled, then the live blocks).
void densify_row(const Lists& L, int r, int cols, float* out);

// The x / h parts of the fatchord step matrices (row-major, leading dimension in floats).
struct StepMatrices {
    const float *wih2, *whh1, *whh2, *fc1, *fc2, *fc3;
    int ld_ih2, ld_hh1, ld_hh2, ld_fc1, ld_fc2, ld_fc3;
    int n_classes;  // rows of fc3: at most 1024
};
// The whole image: per slot the lists of its kSets * kRows rows (set-major), and what
// wrnn_sparse_wide_info reports. fits == false (a slot's lists exceed kCapF4): no image; `slots`
// is empty and the weights run dense.
struct Image {
    std::vector<Lists> slots;
    long long live = 0, total = 0;  // 1 x 4 blocks of the packed sets
    int fill_f4 = 0;                // the fullest slot's blocks
    bool fits = false;
    double density() const { return total ? (double)live / (double)total : 0.0; }
};
Image build_image(const StepMatrices& m);
// The device image of a slot's lists (kSets * kRows rows, at most kCapF4 blocks): kImgWords words,
// zero-filled beyond the lists -- row table (start | count << 16), column words, blocks.
void slot_image(const Lists& L, uint32_t* out);

}  // namespace wsp
}  // namespace wrnn

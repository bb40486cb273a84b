// The block-sparse wide image's packer (sparse_wide_pack.h) and its handle-free debug entry
// points. No HIP: built by g++ like plan.cpp.
#include "sparse_wide_pack.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "wavernn_mi355x.h"

extern "C" int wrnn_internal_fail(int code, const char* msg);  // runtime.hip

namespace wrnn {
namespace wsp {

bool dead4(const float* p) {
    uint32_t w[4];
    std::memcpy(w, p, sizeof w);
    return ((w[0] | w[1] | w[2] | w[3]) & 0x7fffffffu) == 0u;
}

bool append_rows(const float* W, int rows, int ld, int cols, int row0, int nrows, Lists& L) {
    if (cols < 0 || cols / 4 > 65536) return false;
    const size_t rows_before = L.start.size(), blocks_before = L.col.size();
    for (int r = row0; r < row0 + nrows; ++r) {
        const size_t st = L.col.size();
        if (r >= 0 && r < rows)
            for (int c = 0; c + 4 <= cols; c += 4) {
                const float* p = W + (size_t)r * ld + c;
                if (dead4(p)) continue;
                L.blocks.insert(L.blocks.end(), p, p + 4);
                L.col.push_back((uint16_t)(c / 4));
            }
        if (st > 65535u || L.col.size() - st > 65535u) {
            L.start.resize(rows_before);
            L.count.resize(rows_before);
            L.blocks.resize(blocks_before * 4);
            L.col.resize(blocks_before);
            return false;
        }
        L.start.push_back((uint16_t)st);
        L.count.push_back((uint16_t)(L.col.size() - st));
    }
    return true;
}

void densify_row(const Lists& L, int r, int cols, float* out) {
    std::fill(out, out + cols, 0.f);
    for (int i = 0; i < L.count[r]; ++i) {
        const size_t b = (size_t)L.start[r] + i;
        if (4 * (int)L.col[b] + 4 <= cols) std::memcpy(out + 4 * L.col[b], &L.blocks[4 * b], 4 * sizeof(float));
    }
}

Image build_image(const StepMatrices& m) {
    Image im;
    im.slots.resize(kSlots);
    bool fits = true;
    for (int w = 0; w < kSlots; ++w) {
        Lists& L = im.slots[w];
        bool ok = true;
        auto gates = [&](const float* W, int ld) {  // r, z, n: rows j * 512 + 16 w ..
            for (int j = 0; j < 3; ++j) ok = ok && append_rows(W, 3 * kPH, ld, kCols, j * kPH + kRows * w, kRows, L);
        };
        gates(m.wih2, m.ld_ih2);
        gates(m.whh1, m.ld_hh1);
        ok = ok && append_rows(m.fc1, kPH, m.ld_fc1, kCols, kRows * w, kRows, L);
        ok = ok && append_rows(m.fc2, kPH, m.ld_fc2, kCols, kRows * w, kRows, L);
        // (classes at or beyond n_classes: empty lists)
        ok = ok && append_rows(m.fc3, m.n_classes, m.ld_fc3, kCols, kRows * w, kRows, L);
        ok = ok && append_rows(m.fc3, m.n_classes, m.ld_fc3, kCols, kPH + kRows * w, kRows, L);
        gates(m.whh2, m.ld_hh2);
        // blocks of the sets the slot multiplies (fc3: the classes that exist)
        const int fc3_rows = std::max(0, std::min(kRows, m.n_classes - kRows * w)) +
                             std::max(0, std::min(kRows, m.n_classes - kPH - kRows * w));
        im.total += (long long)((kSets - 2) * kRows + fc3_rows) * kColBlocks;
        if (!ok) {
            fits = false;
            continue;
        }
        im.live += L.size();
        im.fill_f4 = std::max(im.fill_f4, L.size());
        fits = fits && L.size() <= kCapF4;
    }
    im.fits = fits;
    if (!fits) im.slots.clear();
    return im;
}

void slot_image(const Lists& L, uint32_t* out) {
    std::fill(out, out + kImgWords, 0u);
    for (size_t r = 0; r < L.start.size() && r < (size_t)(kSets * kRows); ++r)
        out[r] = (uint32_t)L.start[r] | (uint32_t)L.count[r] << 16;
    uint16_t* col = reinterpret_cast<uint16_t*>(out + kTabBytes / 4);
    const size_t n = std::min<size_t>(L.col.size(), kCapF4);
    std::copy(L.col.begin(), L.col.begin() + n, col);
    std::memcpy(out + (kTabBytes + kColBytes) / 4, L.blocks.data(), n * 16);
}

}  // namespace wsp
}  // namespace wrnn

using namespace wrnn;

extern "C" {

int wrnn_debug_wide_sp_pack(const float* W, int rows, int cols, int slot, float* recon, int* sizes, int* total_f4) {
    if (!W) return wrnn_internal_fail(WRNN_ERR_INVALID, "null argument");
    if (rows < kPH || rows % kPH || rows > 3 * kPH || cols < 4 || cols % 4 || cols > wsp::kCols || slot < 0 ||
        slot >= wsp::kSlots)
        return wrnn_internal_fail(WRNN_ERR_INVALID, "bad arguments");
    wsp::Lists L;
    const int parts = rows / kPH;
    for (int j = 0; j < parts; ++j)
        if (!wsp::append_rows(W, rows, cols, cols, j * kPH + wsp::kRows * slot, wsp::kRows, L))
            return wrnn_internal_fail(WRNN_ERR_CAPACITY, "list words");
    for (int r = 0; r < parts * wsp::kRows; ++r) {
        if (recon) wsp::densify_row(L, r, cols, recon + (size_t)r * cols);
        if (sizes) sizes[r] = L.count[r];
    }
    if (total_f4) *total_f4 = L.size();
    return WRNN_OK;
}

int wrnn_debug_wide_sp_image(const float* wih2, int ld_ih2, const float* whh1, const float* whh2, const float* fc1,
                             int ld_fc1, const float* fc2, int ld_fc2, const float* fc3, int n_classes, int* fits,
                             double* density, int* fill_f4) {
    if (!wih2 || !whh1 || !whh2 || !fc1 || !fc2 || !fc3) return wrnn_internal_fail(WRNN_ERR_INVALID, "null argument");
    if (ld_ih2 < kPH || ld_fc1 < kPH || ld_fc2 < kPH || n_classes < 1 || n_classes > 2 * kPH)
        return wrnn_internal_fail(WRNN_ERR_INVALID, "bad arguments");
    const wsp::StepMatrices m{wih2, whh1, whh2, fc1, fc2, fc3, ld_ih2, kPH, kPH, ld_fc1, ld_fc2, kPH, n_classes};
    const wsp::Image im = wsp::build_image(m);
    if (fits) *fits = im.fits ? 1 : 0;
    if (density) *density = im.density();
    if (fill_f4) *fill_f4 = im.fill_f4;
    return WRNN_OK;
}

}  // extern "C"

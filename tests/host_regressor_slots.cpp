// Holds the operand slots of the vertex regressor (gator_amd/csrc/regressor_slots.h) to the fragment indices its kernels form.  Built by
// tests/test_host_regressor_slots.py as plain C++17: the header needs no HIP.  For every layout the loops below walk the packed buffer
// in the order the layout comments of fused_state.h give -- FusedWs::vcp [MT][3][kCB][4][64][4], FusedWs::vcp3 as bf16
// [plane 3][MT][3][28][64][8] or fp16 [MT/4][28][4][3][plane 2][64][8], FusedWs::vcp16 [MT][3][28][64][8], FusedState::up_w3
// [plane 3][tap][ob][28][64][8], up_w2 [ob/2][28][2][tap 3][plane 2][64][8], up_w16 [tap][ob][28][64][8] -- so the running count IS the
// element a kernel reads for (tile, k-step, position | tap, plane, lane, j); lane 32 h + i of a 16-deep fragment holds row i and
// k indices 8 h + j (of a 32-deep fp32 tile: k = 8 g + 4 h + j).  The slot function must name exactly that element for the
// coordinate it stands for.  One line per case: elements walked, slots that differ, fall outside, repeat, and elements never named.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "regressor_slots.h"

using namespace gator;

struct Tally {
    std::vector<unsigned char> seen;
    size_t walked = 0, differ = 0, outside = 0, repeated = 0;
    explicit Tally(size_t elems) : seen(elems, 0) {}
    void at(size_t want, size_t slot) {      // `want`: the element the kernel reads; `slot`: what the function under test names
        ++walked;
        if (slot != want) ++differ;
        if (slot >= seen.size()) { ++outside; return; }
        if (seen[slot]++) ++repeated;
    }
    void report(const char* name, int B, int cap, size_t expect_unnamed) const {
        size_t missed = 0;
        for (unsigned char s : seen) missed += !s;
        printf("%s B=%d cap=%d elems=%zu walked=%zu differ=%zu outside=%zu repeated=%zu unnamed=%zu\n", name, B, cap, seen.size(), walked, differ,
               outside, repeated, missed - expect_unnamed);
    }
};

static void act_f32(int B) {
    const int MT = (B + 31) / 32;
    Tally t(upsample_f32_vcp_elems(B));
    size_t n = 0;
    for (int mt = 0; mt < MT; ++mt) for (int lp = 0; lp < 3; ++lp) for (int cb = 0; cb < 14; ++cb) for (int g = 0; g < 4; ++g)
        for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 4; ++j, ++n)
            t.at(n, act_slot_f32(32 * mt + (lane & 31), 32 * cb + 8 * g + 4 * (lane >> 5) + j, lp));
    t.report("act_f32", B, B, 0);
}

// planes == 3: the three-plane form, planes strided by the capacity's tile count; planes == 1: the bf16 form
static void act_b16(int B, int cap, int planes) {
    const int MT = (B + 31) / 32, MTcap = (cap + 31) / 32;
    const size_t elems = planes == 3 ? upsample_x3_vcp_elems(cap) : upsample_bf16_vcp_elems(B), stride = planes == 3 ? elems / 3 : 0;
    Tally t(elems);
    for (int p = 0; p < planes; ++p) {
        size_t n = (size_t)p * MTcap * 3 * 28 * 64 * 8;
        for (int mt = 0; mt < MT; ++mt) for (int lp = 0; lp < 3; ++lp) for (int s = 0; s < 28; ++s)
            for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 8; ++j, ++n)
                t.at(n, act_slot_b16(32 * mt + (lane & 31), 16 * s + 8 * (lane >> 5) + j, lp) + p * stride);
    }
    // tiles MT .. MTcap of every plane belong to larger batches: nobody names them at this B
    t.report(planes == 3 ? "act_x3" : "act_bf16", B, cap, planes == 3 ? (size_t)3 * (MTcap - MT) * 3 * 28 * 64 * 8 : 0);
}

static void act_x2(int B) {
    const int MG = (B + 127) / 128;
    Tally t(upsample_x2_vcp_elems(B));
    size_t n = 0;
    for (int mg = 0; mg < MG; ++mg) for (int s = 0; s < 28; ++s) for (int mi = 0; mi < 4; ++mi) for (int lp = 0; lp < 3; ++lp)
        for (int p = 0; p < 2; ++p) for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 8; ++j, ++n)
            t.at(n, act_slot_x2(32 * (4 * mg + mi) + (lane & 31), 16 * s + 8 * (lane >> 5) + j, lp) + p * kX2Plane);
    t.report("act_x2", B, B, 0);
}

static void w_b16(int planes) {
    const size_t elems = planes == 3 ? upsample_x3_weight_elems() : upsample_bf16_weight_elems(), stride = planes == 3 ? elems / 3 : 0;
    Tally t(elems);
    size_t n = 0;
    for (int p = 0; p < planes; ++p) for (int tap = 0; tap < 3; ++tap) for (int ob = 0; ob < 216; ++ob) for (int s = 0; s < 28; ++s)
        for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 8; ++j, ++n)
            t.at(n, w_slot_b16(32 * ob + (lane & 31), 16 * s + 8 * (lane >> 5) + j, tap) + p * stride);
    t.report(planes == 3 ? "w_x3" : "w_bf16", 0, 0, 0);
}

static void w_x2() {
    Tally t(upsample_x2_weight_elems());
    size_t n = 0;
    for (int op = 0; op < 108; ++op) for (int s = 0; s < 28; ++s) for (int o2 = 0; o2 < 2; ++o2) for (int tap = 0; tap < 3; ++tap)
        for (int p = 0; p < 2; ++p) for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 8; ++j, ++n)
            t.at(n, w_slot_x2(32 * (2 * op + o2) + (lane & 31), 16 * s + 8 * (lane >> 5) + j, tap) + p * kX2Plane);
    t.report("w_x2", 0, 0, 0);
}

int main() {
    for (int B : {1, 33, 129}) {
        act_f32(B);
        act_x2(B);
        if (B <= 33) act_b16(B, 33, 3);      // a workspace holds at least the batch
        act_b16(B, 257, 3);
        act_b16(B, B, 1);
    }
    w_b16(3);
    w_b16(1);
    w_x2();
    // the tap list: output l = lp + 1 - k inside 0..2, grouped by input position, taps descending
    int n = 0;
    bool ok = true;
    for (int lp = 0; lp < 3; ++lp)
        for (int k = 2; k >= 0; --k) {
            const int l = lp + 1 - k;
            if (l < 0 || l > 2) continue;
            ok = ok && n < 7 && kRegTaps[n].lp == lp && kRegTaps[n].k == k && kRegTaps[n].l == l;
            ++n;
        }
    printf("taps n=%d %s\n", n, ok ? "ok" : "WRONG");
    return 0;
}

// The one statement of how a BA problem's buffers lie in memory: the record
// sizes several translation units index or allocate, and the order, lengths
// and alignment of the float64 segments and of the int32 tail that the window
// staging (winstage.hip) writes and slam355/ba.py allocates.  Every host-side
// consumer gets its numbers from slam_ba_f64_layout / slam_ba_i32_layout
// (winstage.hip), which read this table.
#pragma once

namespace {

constexpr int kCamRec = 32;  // c s omc v(3) R(9) A(9) inv small t(3) f k1 k2 pad(0)
constexpr int kCPart = 112;  // per camera slot: U - sum Y W^T (81), Jc^T r, Jc^T u, diag U (9 each), |r|^2, pad
constexpr int kBPart = 81;   // per block slot: sum Y W^T
constexpr int kSmall = 4;    // trial |r|^2, sum pred_p (all-reduced), two spare

// The float64 segments, in the order they lie in a problem's allocation
// (SLAM_STAGE_NF64 of them): the parameters (two LM copies and the initial
// one) and the observations are uploaded, the rest start as zeros.
enum {
  SLAM_BA_F64_CAMS0 = 0, SLAM_BA_F64_PTS0, SLAM_BA_F64_CAMS1, SLAM_BA_F64_PTS1, SLAM_BA_F64_INIT_C,
  SLAM_BA_F64_INIT_P, SLAM_BA_F64_OBS_Q,
  SLAM_BA_F64_CAMREC0, SLAM_BA_F64_CAMREC1, SLAM_BA_F64_CPART, SLAM_BA_F64_BPART, SLAM_BA_F64_SYS,
  SLAM_BA_F64_CHOL, SLAM_BA_F64_DELTA_C, SLAM_BA_F64_RED_PART, SLAM_BA_F64_SMALL, SLAM_BA_F64_STATE,
  SLAM_BA_F64_COUNT
};
constexpr int kF64Zeroed = SLAM_BA_F64_CAMREC0;  // the first segment that starts as zeros

constexpr long long kBaAlign = 32;  // every segment starts on a multiple of 32 elements (256 B of doubles)
constexpr long long ba_aligned(long long n) { return ((n > 1 ? n : 1) + kBaAlign - 1) / kBaAlign * kBaAlign; }

// The int32 words of a problem: its plan tables, then kI32Tail zero words --
// the one-element stand-ins of the lin_mode-0 tables from +0, the completion
// ticket at +kI32Ticket.
constexpr int kI32Tail = 8;
constexpr int kI32Ticket = 4;

// Length in doubles of every float64 segment.  The parameter segments may be
// empty (no points); a workspace keeps at least one element.
constexpr void ba_f64_lengths(long long C, long long P, long long O, long long n_cslots,
                              long long n_bslots, long long sys_len, long long chol_len,
                              long long red_slots, long long n_state, long long len[SLAM_BA_F64_COUNT]) {
  for (int rep = 0; rep < 3; ++rep) {  // cams0 / pts0, cams1 / pts1, init_c / init_p
    len[2 * rep] = 9 * C;
    len[2 * rep + 1] = 3 * P;
  }
  len[SLAM_BA_F64_OBS_Q] = 2 * (O > 1 ? O : 1);
  len[SLAM_BA_F64_CAMREC0] = len[SLAM_BA_F64_CAMREC1] = kCamRec * C;
  len[SLAM_BA_F64_CPART] = kCPart * n_cslots;
  len[SLAM_BA_F64_BPART] = kBPart * n_bslots;
  len[SLAM_BA_F64_SYS] = sys_len;
  len[SLAM_BA_F64_CHOL] = chol_len;  // the tiled solve's workspace (9C > 120); one element otherwise
  len[SLAM_BA_F64_DELTA_C] = 9 * C;
  len[SLAM_BA_F64_RED_PART] = red_slots;
  len[SLAM_BA_F64_SMALL] = kSmall;
  len[SLAM_BA_F64_STATE] = n_state;
  for (int k = kF64Zeroed; k < SLAM_BA_F64_COUNT; ++k)
    if (len[k] < 1) len[k] = 1;
}

}  // namespace

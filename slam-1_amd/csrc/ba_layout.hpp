// Record sizes of the BA buffers that several translation units index or
// allocate (the BA files, and winstage.hip for the window staging arena).
#pragma once

namespace {

constexpr int kCamRec = 32;  // c s omc v(3) R(9) A(9) inv small t(3) f k1 k2 pad(0)
constexpr int kCPart = 112;  // per camera slot: U - sum Y W^T (81), Jc^T r, Jc^T u, diag U (9 each), |r|^2, pad

}  // namespace

// The sizes the texture and track units agree on, ONE definition of each (texture_ops.hip, track_ops.hip, track_stream.hip,
// track_link.hip, track_reid.hip).
#pragma once

namespace danet {

constexpr int kNB = 10;                          // betas of a row
constexpr int kParaRow = 3 + kNB + 216;          // 229: cam, betas, 24 rotation matrices
constexpr int kParts = 24;                       // DensePose charts of an atlas

}  // namespace danet

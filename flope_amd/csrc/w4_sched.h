// The hand-counted part of conv_w4's schedule (conv_w4.hip), in ONE place: which vector-memory operations a wave issues where, and
// the `s_waitcnt vmcnt(N)` it executes in front of each workgroup barrier.  The kernel takes its counts from w4_wait_n() -- a small
// constexpr MODEL of the wave's in-order memory queue, not a closed formula -- and the host-side check
// (tests/host_harness/harness.cpp: flope_host_w4_schedule_check, tests/test_host.py) replays the same model against an
// independent statement of what must have landed where.  (r03 found a count that was one burst too lax by re-deriving it on paper --
// timing had always hidden it; VERDICT r3 item 5.  The r03 closed forms are kept below as w4_wait_n_r03* for that test.)
//
// Vocabulary.  A tile's K loop is a sequence of BODIES (64 input channels each); a body is 9 DOUBLE STEPS D = 0..8 = 18
// SUB-STEPS u = 2 D, 2 D + 1 (sub-step u = tap u % 9 of half-chunk u / 9: 32-channel patch buffer u / 9).  Barrier D sits BETWEEN the
// two sub-steps of double step D.  Per double step a wave consumes one DOUBLE TILE of weights (ring slot) and issues, in the SECOND
// sub-step (behind the barrier), in this order:
//   W4_TGW pieces of double tile D + PD (PD = ring depth - 1) into the slot PD ahead, then
//   w4_patch_pieces(D, PW, spread) pieces of a patch burst (PW = pieces per burst = 2 PT):
//     buffer 1 <- this body's second half-chunk: all PW pieces at D = 0.  First read: the fragments of sub-step 9, fetched during
//                 sub-step 8 = the first sub-step of D = 4, i.e. behind barrier 3.  (Free since barrier 8 of the previous body.)
//     buffer 0 <- the NEXT body's (class walk: next tile's) first half-chunk: all PW pieces at D = 5 (spread <= 1), or in `spread`
//                 parts at D = 4, 5, ...  First read: the fragments of the next body's sub-step 0, fetched during sub-step 17 = the
//                 second sub-step of D = 8, behind barrier 8.  (Free since barrier 4: its last fragments -- sub-step 8's -- are
//                 fetched during sub-step 7 and are in registers when a wave reaches barrier 4.)
//   r04, why spread: this burst reads lines nobody has touched (the second 128 bytes of every pixel, or the next tile), every
//   workgroup of the launch issues it in the same microsecond, and a wave's memory operations RETURN IN ORDER -- the weight pieces
//   issued behind a cold burst (L2 hits) cannot complete until it has, the return path fills and the wave's next DMA issue blocks
//   with the matrix pipe idle: 750 - 1000 cycles per weight piece in the double step behind the burst, ~3 k cycles per cold burst
//   (profiles/r04_conv_w4_cold_burst_stamps.txt).  Parts must still be issued >= 3 double steps ahead of barrier 8.
// In front of barrier D the wave waits until everything that is read behind that barrier has landed: double tile D + 1, and the
// patch bursts that are due (buffer 1 from barrier 3 on, buffer 0 at barrier 8).  Operations return in issue order, so the count is
// "how many operations were issued behind the youngest one that must have landed".
#pragma once

#include <stddef.h>

#ifndef W4_HD
#if defined(__HIPCC__)
#define W4_HD __host__ __device__
#else
#define W4_HD
#endif
#endif

#define W4_TGW 4   // LDS-DMA operations per wave per double tile (16 KB / 4 waves / 1 KB)

// weight-ring depth (double tiles) of a variant: the deepest of 5, 4, 3 that fits the CU's 160 KB beside two patch buffers of PT
// 8 KB rounds, the 12.5 KB scratch and (class walk + folded shortcut) the shortcut's own weight slot; 0 = does not fit
W4_HD constexpr int w4_ring(int pt, bool own_ds_slot) {
  for (int n = 5; n >= 3; --n)
    if (2 * pt * 8192 + (n + (own_ds_slot ? 1 : 0)) * 16384 + 12800 <= 160 * 1024) return n;
  return 0;
}

// LDS bytes of a variant: 2 patch buffers, the weight ring (+ 1 double tile for a persistent workgroup's folded shortcut), 12.5 KB in
// which the lanes trade their shares of the address table and the epilogue builds its line image
W4_HD constexpr size_t w4_lds_bytes(int pt, bool own_ds_slot) {
  return (size_t)2 * pt * 8192 + (size_t)(w4_ring(pt, own_ds_slot) + (own_ds_slot ? 1 : 0)) * 16384 + 12800;
}

// patch pieces a wave issues in the second sub-step of double step D, and the burst index of the first of them.
// spread <= 1: the buffer-0 burst whole at D = 5; spread = 2, 3, 4: in that many parts at D = 4, 5, .. (PW = 8, 2 parts: 4 4;
// 3 parts: 3 3 2; PW = 10, 2 parts: 5 5; PW = 12, 3 parts: 4 4 4)
W4_HD constexpr int w4_patch_pieces(int D, int PW, int spread) {
  if (D == 0) return PW;
  if (spread <= 1) return D == 5 ? PW : 0;
  if (D < 4 || D >= 4 + spread) return 0;
  return PW / spread + ((D - 4) < PW % spread ? 1 : 0);
}
W4_HD constexpr int w4_patch_first(int D, int PW, int spread) {
  int j = 0;
  if (spread > 1) for (int d = 4; d < D; ++d) j += w4_patch_pieces(d, PW, spread);
  return (D == 0 || spread <= 1) ? 0 : j;
}
// which patch buffer the pieces of double step D fill (0 / 1), or -1
W4_HD constexpr int w4_patch_buffer(int D, int PW, int spread) { return w4_patch_pieces(D, PW, spread) == 0 ? -1 : (D == 0 ? 1 : 0); }
// DMA pieces of the second sub-step of double step D
W4_HD constexpr int w4_pieces(int D, int PW, int spread, int tgw = W4_TGW) { return tgw + w4_patch_pieces(D, PW, spread); }

// Class walk + residual input, LAST body: the tile's 2 MT residual loads (register loads by inline assembly) are issued in the FIRST
// sub-steps of double steps 7 (8 loads) and 8 (the other 2 MT - 8), i.e. right in front of the waits of barriers 7 and 8.
W4_HD constexpr int w4_res_loads(int D, int MT) { return D == 7 ? 8 : (D == 8 ? 2 * MT - 8 : 0); }
W4_HD constexpr int w4_res_first(int MT) { return 8; }            // index of the first load of double step 8

// ---- the queue model.  Operations of a wave in issue order over TWO consecutive bodies (the one before and the current one), with
// `boundary_ops` operations between them (class walk: the 2 MT epilogue stores of a tile boundary; 0 inside a tile) and, when res_mt >
// 0, the residual loads of the current body's first sub-steps 7 and 8 (class walk, last body).  Returns vmcnt for barrier D of the
// current body: the number of operations issued behind the youngest one that has to have landed there.
//   needed at barrier D of the current body: double tiles <= D + 1 of the current body (and everything of the body before: its
//   double tiles were read there, its buffer-1 burst was due at its barrier 3, its buffer-0 burst at its barrier 8), this body's
//   buffer-1 burst from D = 3 on, this body's buffer-0 pieces at D = 8.  Double tile k of the current body is issued at double step
//   k - PD of the current body, or (k < PD) at double step 9 + k - PD of the body before.
// (tgw: pieces of a double tile per wave -- 4 on the 4-wave kernel; r04's 8-wave experiment used 2)
W4_HD constexpr int w4_wait_n(int D, int PD, int PW, int spread, int boundary_ops, int res_mt, int tgw = W4_TGW) {
  int issued = 0, last_needed = 0;                       // running count of issued operations; 1-based index of the youngest needed one
  // body -1 (everything needed; its double tiles 9 .. belong to the current body: index k = d + PD - 9)
  for (int d = 0; d < 9; ++d) {
    for (int i = 0; i < tgw; ++i) { ++issued; const int k = d + PD - 9; if (k <= D + 1) last_needed = issued; }
    for (int i = 0; i < w4_patch_pieces(d, PW, spread); ++i) { ++issued; last_needed = issued; }
  }
  issued += boundary_ops;
  // current body: double steps 0 .. D - 1 have issued their second sub-steps; first sub-steps 0 .. D theirs
  for (int d = 0; d <= D; ++d) {
    issued += res_mt > 0 ? w4_res_loads(d, res_mt) : 0;  // first sub-step of d (in front of barrier d): never needed by a barrier
    if (d == D) break;
    for (int i = 0; i < tgw; ++i) { ++issued; if (d + PD <= D + 1) last_needed = issued; }
    const int buf = w4_patch_buffer(d, PW, spread);
    for (int i = 0; i < w4_patch_pieces(d, PW, spread); ++i) { ++issued; if ((buf == 1 && D >= 3) || (buf == 0 && D >= 8)) last_needed = issued; }
  }
  return issued - last_needed;
}

// r03's closed forms (spread = 0), kept for the schedule test: the shipped one, and the one r03 replaced after finding it a burst too
// lax at barriers 3 and 8 of a 5-deep ring
W4_HD constexpr int w4_wait_n_r03(int D, int PD, int PW) {
  return W4_TGW * (PD - 2) + (((D >= 1 && D <= PD - 1 && D <= 2) || (D >= 6 && D <= PD + 4 && D <= 7)) ? PW : 0);
}
W4_HD constexpr int w4_wait_n_r03_lax(int D, int PD, int PW) {
  return W4_TGW * (PD - 2) + (((D >= 1 && D <= PD - 1) || (D >= 6 && D <= PD + 4)) ? PW : 0);
}

// The per-row arithmetic of flope_frame_select (frame.hip: frame_select_kernel), in ONE place and without HIP: how many detector
// rows the kernel reads, and what it decides about each.  The kernel takes both from here and keeps only its ballots and ranks;
// tests/host_harness/harness_frame.cpp exports the same functions to the CPU tests (tests/frame_cases.py,
// tests/test_frame_cases.py), which compare them with the two Python statements of the reference's loop.
//
// The operation (fast_pose_predictor.py:55-56, :65-83; mvg.py:324-351): float32 xyxy -> int16 as numpy's astype does it
// (truncation toward zero), squarify_bb -- the short side grows to the long one, its min edge moves by ceil(d / 2) and its max
// edge by floor(d / 2), nothing is clamped -- and bb_in_frame: the square is kept unless xmin < 0, ymin < 0, xmax > W or ymax > H
// (xmax == W and ymax == H are accepted).  Nothing here asks for x1 > x0 or y1 > y0: an inverted box has w < 0 or h < 0, is squared
// by the same rule (so its x edges may land in the frame) and is kept or dropped by the same four comparisons; a zero-area box in
// the frame is kept.  What a kept box of that kind selects is defined downstream: empty and inverted ranges select nothing in the
// depth lift (depth_plan.h) and give an all-zero crop (crop_plan.h).
//
// Domain: finite coordinates with |v| <= 32767.  A detector that clips its boxes to a frame the handle accepts (at most 32767 x
// 32767) gives nothing else.  Beyond that both C's float -> int conversion and numpy's astype(int16) are undefined, and no test
// goes there.
#pragma once

#ifndef FRAME_HD
#if defined(__HIPCC__)
#define FRAME_HD __host__ __device__
#else
#define FRAME_HD
#endif
#endif

constexpr int kFrameDetRow = 8;            // floats per detector row: x0, y0, x1, y1, then what the selection never reads

// rows the kernel reads: the detector's count, clamped to the table it was given
FRAME_HD inline int frame_count(int count, int max_det) { return count < 0 ? 0 : (count > max_det ? max_det : count); }

// one coordinate: float32 -> int16 like numpy's astype (truncation toward zero: -0.999 is 0, -1.0 is -1)
FRAME_HD inline int frame_coord(float v) { return (int)(short)(int)v; }

// row = x0, y0, x1, y1 of one detection in a frame of W x H -> good = the int16 box as detected, sq = its square; true: the square
// lies inside the frame and the box is kept
FRAME_HD inline bool frame_box(const float* row, int W, int H, int good[4], int sq[4]) {
  const int x0 = frame_coord(row[0]), y0 = frame_coord(row[1]), x1 = frame_coord(row[2]), y1 = frame_coord(row[3]);
  const int w = x1 - x0, h = y1 - y0, d = w > h ? w - h : h - w;
  const int lo = (d + 1) / 2, hi = d / 2;                         // the min edge moves by ceil(d / 2), the max edge by floor(d / 2)
  good[0] = x0; good[1] = y0; good[2] = x1; good[3] = y1;
  sq[0] = x0; sq[1] = y0; sq[2] = x1; sq[3] = y1;
  if (w > h) { sq[1] -= lo; sq[3] += hi; } else if (h > w) { sq[0] -= lo; sq[2] += hi; }
  return !(sq[0] < 0 || sq[1] < 0 || sq[2] > W || sq[3] > H);     // xmax == W and ymax == H are accepted
}

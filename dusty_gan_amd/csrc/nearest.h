// The NEAREST resize rule of the dataset's transform, written once: dg_scan_to_polar (lidar_io.hip) resamples a projected scan
// with it and dg_label_resize (object_removal.hip) the scan's label image, so a pixel and its label come from the same cell.
#pragma once

// torch's legacy "nearest" (what torchvision 0.9 TF.resize(tensor, size, NEAREST) calls: F.interpolate(mode="nearest")):
// src = min(floor(dst * float(in) / out), in - 1)
__device__ __forceinline__ int nearest_src(int dst, int in_size, int out_size) {
  const float scale = (float)in_size / (float)out_size;
  const int s = (int)floorf((float)dst * scale);
  return s < in_size - 1 ? s : in_size - 1;
}

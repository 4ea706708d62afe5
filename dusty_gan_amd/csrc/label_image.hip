// Semantic labels on the range image (gfx950; dusty_gan_amd/datasets/labels.py): the SemanticKITTI branch of the
// reference's process_kitti.py (:120-131), which scatters the mapped label of every point far-to-near exactly as it scatters
// the points.  Here no second scatter runs: dg_scan_project / dg_beam_project leave in `keys` the z-buffer word of every cell
// (range bits << 32 | the winner's index within its scan, or KEY_EMPTY), and the label image is read through those words - the
// label of the very record the projection's `out` holds, by construction, with the projection's tie rule (the LOWER index
// on equal float32 ranges; the reference's unstable argsort leaves ties undefined).
//   sem    lut[labels[offsets[s] + winner] & 0xFFFF]  (the reference's labelmap.__getitem__), 0 for an empty cell
//   inst   labels >> 16 of the winner (SemanticKITTI's instance id), 0 for an empty cell
//   status |= 1 for a scan one of whose WINNERS carries an id the table does not know (lut = 255).  The reference raises a
//          KeyError for such an id on any point; a point that wins no cell does not reach the image and is not looked at here.
// One launch, one thread per cell: 8 bytes of key and one gathered label word in, 1 (+ 2) bytes out; the table's 64 KiB stay
// in L2.  The only atomic is an integer OR on the scan's status word.
#include "common.h"
#include "scan_cell.h"

namespace {

__global__ __launch_bounds__(256) void scan_labels_kernel(const unsigned long long* __restrict__ keys,
                                                          const long* __restrict__ offsets, const unsigned* __restrict__ labels,
                                                          const unsigned char* __restrict__ lut, long cells_per_scan, long n,
                                                          unsigned char* __restrict__ sem, unsigned short* __restrict__ inst,
                                                          int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = (int)(i / cells_per_scan);
  const unsigned long long k = keys[i];
  unsigned char c = 0;
  unsigned short in = 0;
  if (k != KEY_EMPTY) {
    const long o0 = offsets[s], idx = (long)(unsigned)(k & 0xFFFFFFFFull);
    if (idx < offsets[s + 1] - o0) {   // (scan_gather_kernel's guard: a winner is never an address outside its scan)
      const unsigned word = labels[o0 + idx];
      c = lut[word & 0xFFFFu];
      in = (unsigned short)(word >> 16);
      if (c == 255) atomicOr(&status[s], 1);
    }
  }
  sem[i] = c;
  if (inst) inst[i] = in;
}

}  // namespace

extern "C" {

int dg_scan_labels(const unsigned long long* keys, const long* offsets, const unsigned* labels, const unsigned char* lut, int S,
                   int H, int W, unsigned char* sem, unsigned short* inst, int* status, void* s_) {
  if (!keys || !offsets || !labels || !lut || !sem || !status || S < 1 || H <= 0 || W <= 0) return DG_EINVAL;
  if ((long)H * W > 0x7FFFFFFFl) return DG_EINVAL;
  const long cells = (long)H * W, n = (long)S * cells;
  scan_labels_kernel<<<sc_nblk(n), 256, 0, (hipStream_t)s_>>>(keys, offsets, labels, lut, cells, n, sem, inst, status);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"

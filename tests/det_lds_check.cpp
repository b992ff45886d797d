// The LDS layouts of det_match_kernel and det_confusion_kernel (csrc/det_common.h) against the closed forms their sizes had when host and
// kernel stated them separately, and against the arrays' element sizes: a stand-alone host program, compiled for the host alone.
#include <cstdio>

#include "det_common.h"

static int slots(int G) { return (G + 1) & ~1; }

int main() {
  const int dets[] = {1, 255, 256, 257, 16384}, gts[] = {0, 1, 2, 1023, 1024};
  long long cases = 0, bad = 0;
  for (int max_det : dets)
    for (int G : gts) {
      const det_match_layout m = det_match_layout_of(max_det, G);
      const det_confusion_layout c = det_confusion_layout_of(max_det, G);
      const size_t m_total = 32 + (size_t)32 * slots(G) + (size_t)8 * ((max_det + 3) & ~3);
      const size_t c_total = (size_t)36 * slots(G) + (size_t)4 * max_det;
      std::printf("max_det %5d G %4d: det_match %zu (closed form %zu), det_confusion %zu (closed form %zu)\n", max_det, G, m.total, m_total, c.total,
                  c_total);
      bad += m.total != m_total || c.total != c_total;
      // every array holds its elements and starts where its type may start: 8-byte keys, 4-byte ints and floats
      bad += m.best < 4 * 8 || m.gbox < m.best + (size_t)8 * G || m.match < m.gbox + (size_t)24 * G ||
             m.qscore < m.match + (size_t)4 * max_det || m.total < m.qscore + (size_t)4 * max_det || m.best % 8 || m.gbox % 4 || m.match % 4 ||
             m.qscore % 4;
      bad += c.top != 0 || c.gbox < c.top + (size_t)8 * G || c.winner < c.gbox + (size_t)24 * G || c.choice < c.winner + (size_t)4 * G ||
             c.total < c.choice + (size_t)4 * max_det || c.gbox % 4 || c.winner % 4 || c.choice % 4;
      ++cases;
    }
  if (bad) {
    std::printf("det_lds_check: %lld mismatches\n", bad);
    return 1;
  }
  std::printf("det_lds_check: %lld cases ok\n", cases);
  return 0;
}

// Training hot path of libanirec for gfx950 (MI355X): the head kernel that also accumulates the Keras metrics,
// k_head_metrics — one instantiation per (activation, loss) pair, a unit of its own only because it is a third of the
// training path's device code.  launch_head (anirec_train_head.hip) hands the launches with a metric set over.
#include <hip/hip_runtime.h>

#include "anirec_train_head.hpp"
#include "anirec_train_lazy.hpp"

namespace anirec {

// the same launch with the Keras metrics of m (anirec_trainer_set_metrics / anirec_dist_stepper_set_metrics).  ALL of
// its LDS is one array — the block-sum scratch, then the AUC histogram — since a second __shared__ object can make
// hipcc wait vmcnt(0) in front of LDS accesses (the histogram is zeroed before the first barrier of head_block)
template <int kAct, int kLoss>
__global__ __launch_bounds__(kHeadThreads) void k_head_metrics(HeadArgs a, LazyArgs z, int n_head, MetricArgs m) {
  __shared__ float lds[kHeadCols * 16 + 2 * kAucBins];
  tick(a.ticks, 0);
  const anirec_state *st = a.state;
  if ((int)blockIdx.x >= n_head) {  // (the catch-up workgroups as in k_head)
    const int step = st->step_fwd, w0 = z.w0[0];
    if (step + 1 < z.n_steps && step + 1 - w0 <= kLzWin)
      lazy_catchup_row(z, step + 1, w0, z.cu_lo + (int)blockIdx.x - n_head, step + 1);
    tick(a.ticks, 1);
    return;
  }
  if (m.mask & ANIREC_METRIC_AUC) {
    for (int k = threadIdx.x; k < 2 * kAucBins; k += kHeadThreads) lds[kHeadCols * 16 + k] = 0.f;  // (0.f: 0u)
  }
  const HeadIn in = {st->step_fwd, st->w, st->b, st->gamma, st->beta};
  head_block<kAct, kLoss, true>(a, in, blockIdx.x, n_head, lds, m);
  tick(a.ticks, 1);
}

// the head launch with a metric set: the arguments, the grid and the stamps are launch_head's
void launch_head_metrics(const anirec_train_desc *d, const HeadArgs &a, const LazyArgs &z, int n_head, int extra,
                         MetricArgs m, hipStream_t s) {
  with_act(d->activation, [&](auto act) {
    with_loss(d->loss, [&](auto loss) {
      hipLaunchKernelGGL((k_head_metrics<decltype(act)::value, decltype(loss)::value>), dim3(n_head + extra),
                         dim3(kHeadThreads), 0, s, a, z, n_head, m);
    });
  });
}

}  // namespace anirec

// Training hot path of libanirec for gfx950 (MI355X): the head kernel of the step, k_head — one instantiation per
// (activation, loss) pair, a quarter of the training path's device code — and launch_head, the head launch of every
// caller.  The launch with a metric set is anirec_train_head_metrics.hip's.
#include <hip/hip_runtime.h>
#include <string.h>

#include "anirec_train_head.hpp"
#include "anirec_train_lazy.hpp"

namespace anirec {

// head(t) — and, lazy dense Adam with the next batch already prepared (n_head < gridDim.x), beside it the catch-up of
// the rows of batch t + 1 that batch t does NOT touch (fwd(t) marked its rows): workgroups [n_head, gridDim.x) bring
// them up to step t + 1 while the forty head workgroups, bwd and the sparse step of batch t run — the rows are
// disjoint from everything those read or write, so no order between them matters, and the next step starts at fwd.
// (Step t itself is an L2-only step for them.)  Round 3 ran this catch-up as the second half of k_lazy_adam(t), on
// the critical path behind bwd: 19 us for that launch; here it hides behind a head launch that used 40 of 256 CUs.
template <int kAct, int kLoss>
__global__ __launch_bounds__(kHeadThreads) void k_head(HeadArgs a, LazyArgs z, int n_head) {
  __shared__ float scratch[kHeadCols * 16];
  tick(a.ticks, 0);
  const anirec_state *st = a.state;
  if ((int)blockIdx.x >= n_head) {
    const int step = st->step_fwd, w0 = z.w0[0];
    if (step + 1 < z.n_steps && step + 1 - w0 <= kLzWin)
      lazy_catchup_row(z, step + 1, w0, z.cu_lo + (int)blockIdx.x - n_head, step + 1);
    tick(a.ticks, 1);
    return;
  }
  const HeadIn in = {st->step_fwd, st->w, st->b, st->gamma, st->beta};
  head_block<kAct, kLoss>(a, in, blockIdx.x, n_head, scratch);
  tick(a.ticks, 1);
}

static HeadArgs head_args(const anirec_train_desc *d, const TrainWs &w) {
  HeadArgs a;
  a.state = d->state;
  a.sched = d->sched;
  a.packets = d->packets;
  a.packet_floats = anirec_packet_floats(d->max_batch);
  a.n_seg = d->n_seg;
  a.my_seg = d->my_seg;
  a.cap = d->max_batch;
  a.arena_steps = d->arena_steps;
  a.dy = w.dy;
  a.hpart = w.hpart;
  a.hpart_stride = w.hpart_stride;
  a.pub = w.pub;
  a.sel = w.sel;
  a.l2 = d->l2;
  a.ticks = ticks_of(w, 1);
  return a;
}

static inline int head_blocks(const anirec_train_desc *d) {
  return (d->max_batch + kHeadThreads - 1) / kHeadThreads * d->n_seg;
}

// fuse_next (lazy update, the next batch's chunk table is in the arena): the launch also carries the catch-up
// workgroups of that batch's rows.  m.mask != 0: the metrics instantiation (k_head_metrics, launched by its own unit)
int launch_head(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, bool fuse_next, MetricArgs m) {
  const HeadArgs a = head_args(d, w);
  const int nh = head_blocks(d);
  LazyArgs z;
  memset(&z, 0, sizeof(z));
  int extra = 0;
  if (fuse_next && d->lazy != 0 && d->lazy_state != nullptr) {
    z = lazy_args(d, w, 1);
    z.ticks = nullptr;  // (the head's own stamps cover every workgroup of the launch)
    extra = catchup_head_share(d, w);
  }
  // the output head is a template parameter: the default pair's instantiation is the kernel as it always was
  if (m.mask) {
    launch_head_metrics(d, a, z, nh, extra, m, s);
  } else {
    with_act(d->activation, [&](auto act) {
      with_loss(d->loss, [&](auto loss) {
        hipLaunchKernelGGL((k_head<decltype(act)::value, decltype(loss)::value>), dim3(nh + extra),
                           dim3(kHeadThreads), 0, s, a, z, nh);
      });
    });
  }
  if (int te = ticks_collect(w, 1, s)) return te;
  return (int)hipGetLastError();
}

}  // namespace anirec

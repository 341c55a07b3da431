// voxe_ray_loss.hpp -- what the density ray losses share around the sample march ("What the ray
// losses share"): voxe_distortion.hip, voxe_depth.hip and voxe_orientation.hip.
//
// Each of them marches the forward's samples over the raw densities (voxe_ray_march.hpp) with G lanes per ray and returns the
// mean over the rays of omega_r L_r, optionally L_r per ray, and a density gradient deposited with float atomics.  A loss
// supplies its kernel -- the phases and the maths of L_r, top to bottom -- and a launch_* that hands launch_ray_loss() the
// kernel launch; the kernel ends its value part in ray_loss_outputs() and deposits a sample's gradient with deposit_corners().
#pragma once

#include "voxe_launch.hpp"
#include "voxe_ray_march.hpp"

namespace voxe {

// The value outputs of a ray whose G lanes all hold its L_r: ray_loss[r] = L_r, and partial[block] = the block's sum of
// omega_r L_r (fixed order; launch_partial_mean() turns the partials into the mean).  Every thread of the block calls it.
__device__ __forceinline__ void ray_loss_outputs(bool valid, int j, long long r, double Ltot, float omega,
                                                 float* __restrict__ ray_loss, double* __restrict__ partial) {
  if (valid && j == 0 && ray_loss) ray_loss[r] = (float)Ltot;
  if (partial) {
    const double s = block_sum((valid && j == 0) ? (double)omega * Ltot : 0.0);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
  }
}

// The gradient of one sample on the 8 corners of its cell: term(q) * pre'(raw_q), one float atomic per corner; adding exact
// zeros is skipped
template <class Term>
__device__ __forceinline__ void deposit_corners(const DevGrid& g, const DensityTaps& tp, float* d_dens, Term&& term) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float gq = term(q) * pre_activate_grad(g.pre_act, tp.raw[q], g.density_scale);
    if (gq != 0.0f) atomicAdd(d_dens + tp.idx[q], gq);
  }
}

// The launch of a ray loss: G = lanes_per_ray(R, pinned_lanes), GRAD = a gradient is wanted, the blocks of WaveRectTile<G>,
// the gradient's scale grad_scale / R and the partials in `scratch` (ray_loss_scratch_bytes(); none without loss_out) go to
//   launch(std::integral_constant<int, G>, std::bool_constant<GRAD>, nb, gscale, partial),
// which launches the loss's kernel; then the mean of the partials
template <class Launch>
void launch_ray_loss(const DevCfg& c, int pinned_lanes, float grad_scale, float* loss_out, const float* d_dens, void* scratch,
                     hipStream_t st, Launch&& launch) {
  const float gscale = (float)((double)grad_scale / (double)c.R);
  double* partial = loss_out ? (double*)scratch : nullptr;
  long long nb = 0;
  for_lanes(lanes_per_ray(c.R, pinned_lanes), [&](auto G) {
    nb = group_blocks<WaveRectTile<G()>>(c);
    if (d_dens) launch(G, std::true_type{}, nb, gscale, partial);
    else launch(G, std::false_type{}, nb, gscale, partial);
  });
  if (loss_out) launch_partial_mean(partial, nb, c.R, loss_out, st);
}

}  // namespace voxe

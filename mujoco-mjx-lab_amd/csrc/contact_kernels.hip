// Contact readout (mjl_forward_contacts): the contact list and per-contact forces of a forward pass.
//
// The forward pass of the call runs with its constraint rows in the env's slab of global scratch
// (step_kernel<D, MODE_FORWARD> with force_global_rows, bit-identical to the LDS path), which leaves
// there everything Data.contact and mj_contactForce hold: the contact records (pos, frame, mu, the
// packed bodies / condim), the pair and first-row index of each contact, and the rows' epos and force.
// contacts_kernel reads that slab through global_rows<D>() and the contact count from the stats row the
// forward stored; it changes nothing the forward wrote. One wavefront per env:
//   pos, frame        the first 12 floats of each CONW-float record; the env's output block is
//                     contiguous, so consecutive lanes store consecutive floats (as copy_rows)
//   geom, dim, efc_adr, dist, force     lane = contact, in trips of 64
//   body_force        lane = body, one wave-uniform loop over ALL the env's contacts in contact
//                     order: a fixed summation order, no atomics, independent of max_con
// Entries from the env's contact count up to max_con get the sentinel (geom -1, the rest 0) in the
// same loops. No LDS, no cross-lane traffic.
// Included by capi.hip after step_kernels.hip (Rows / global_rows, the model records, wave primitives).
#pragma once

namespace mjl {

struct ContactOut {  // mjl_forward_contacts' output buffers (each but ncon may be null), by value
  int *ncon, *geom, *dim, *efc_adr;
  float *dist, *pos, *frame, *force, *body_force;
  int max_con;
};

// contact-frame force (normal, tangent 1, tangent 2) of a contact whose first row is r0 [mj_contactForce]:
// a condim-1 contact has one row; a pyramidal one four, J = n + mu t1, n - mu t1, n + mu t2, n - mu t2
// (build_rows), so the normal force is the rows' sum (in row order, as `sensors` adds it) and the
// tangential ones the differences times mu
static INL void contact_frame_force(const Rows<true>& R, int r0, int dim, float mu, float* f) {
  const float f0 = R.force[r0];
  f[0] = f0; f[1] = 0.f; f[2] = 0.f;
  if (dim != 1) {
    const float f1 = R.force[r0 + 1], f2 = R.force[r0 + 2], f3 = R.force[r0 + 3];
    f[0] = ((f0 + f1) + f2) + f3;
    f[1] = (f0 - f1) * mu;
    f[2] = (f2 - f3) * mu;
  }
}
// a contact's first row, kept inside the slab whatever the slab holds
static INL int contact_row0(const Rows<true>& R, int c, int dim) {
  const int nrow = dim == 1 ? 1 : 4;
  return max(0, min(R.con_efc[c], R.cap - nrow));
}

template <class D>
__global__ __launch_bounds__(64) void contacts_kernel(const ModelF* mg, const float* stats, const float* mask,
                                                      float* scratch, int scratch_stride, int gmax_efc, int gmax_con,
                                                      int nenv, ContactOut O) {
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= nenv) return;
  if (mask && !(mask[env] > 0.5f)) return;  // the forward skipped this env: its slab is stale
  MP m = uniform_ptr((MP)mg);
  const Rows<true> R = global_rows<D>(scratch + (size_t)env * (size_t)scratch_stride, gmax_efc, gmax_con);
  const int ncon = uni_int((int)stats[(size_t)env * 4]);
  const int nslab = max(0, min(ncon, gmax_con));  // contacts in the slab (the forward never emits more)
  const int mc = O.max_con, n = min(nslab, mc);
  const size_t e0 = (size_t)env * (size_t)mc;
  if (lane == 0) O.ncon[env] = ncon;

  if (O.pos) {
    GLBA float* o = (GLBA float*)O.pos + e0 * 3;
    for (long i = lane; i < (long)mc * 3; i += 64) o[i] = i < n * 3 ? R.con[((int)i / 3) * CONW + (int)i % 3] : 0.f;
  }
  if (O.frame) {
    GLBA float* o = (GLBA float*)O.frame + e0 * 9;
    for (long i = lane; i < (long)mc * 9; i += 64) o[i] = i < n * 9 ? R.con[((int)i / 9) * CONW + 3 + (int)i % 9] : 0.f;
  }
  if (O.geom || O.dim || O.efc_adr || O.dist || O.force) {
    for (long c = lane; c < mc; c += 64) {  // (long: max_con is the caller's, any positive int)
      int g1 = -1, g2 = -1, dim = 0, r0 = 0;
      float dist = 0.f, f[3] = {0.f, 0.f, 0.f};
      if (c < n) {
        const GLBA float* cr = R.con + (int)c * CONW;
        dim = (__float_as_int(cr[15]) >> 16) & 0xff;
        r0 = contact_row0(R, (int)c, dim);
        const PairRec pr = ldrec(&m->prec[max(0, min(R.con_pair[c], MJL_MAXPAIR - 1))]);
        g1 = pr.g1; g2 = pr.g2;
        dist = R.epos[r0] + pr.includemargin;  // the rows hold dist - includemargin
        contact_frame_force(R, r0, dim, cr[14], f);
      }
      if (O.geom) { O.geom[(e0 + c) * 2] = g1; O.geom[(e0 + c) * 2 + 1] = g2; }
      if (O.dim) O.dim[e0 + c] = dim;
      if (O.efc_adr) O.efc_adr[e0 + c] = r0;
      if (O.dist) O.dist[e0 + c] = dist;
      if (O.force) { for (int k = 0; k < 3; k++) O.force[(e0 + c) * 3 + k] = f[k]; }
    }
  }
  if (O.body_force) {
    // F = frame^T force in the world, +F on geom2's body, -F on geom1's: the normal points from geom1
    // to geom2 and the rows' Jacobian is (body 2's point velocity) - (body 1's) (build_rows)
    const int nbody = m->nbody;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < nslab; c++) {  // uniform: every lane reads the same contact
      const GLBA float* cr = R.con + c * CONW;
      const int packed = __float_as_int(cr[15]), dim = (packed >> 16) & 0xff;
      const int b1 = packed & 0xff, b2 = (packed >> 8) & 0xff;
      float f[3];
      contact_frame_force(R, contact_row0(R, c, dim), dim, cr[14], f);
      for (int k = 0; k < 3; k++) {
        const float F = cr[3 + k] * f[0] + cr[6 + k] * f[1] + cr[9 + k] * f[2];
        if (lane == b2) acc[k] += F;
        if (lane == b1) acc[k] -= F;
      }
    }
    if (lane < nbody) {
      for (int k = 0; k < 3; k++) O.body_force[((size_t)env * nbody + lane) * 3 + k] = acc[k];
    }
  }
}

}  // namespace mjl

// Device code of the centroidal readout that more than one kernel runs: a subtree's mass and centre of mass out
// of the per-body table, the set of bodies a dof moves inside a subtree, and the dof's column of the centre-of-mass
// Jacobian (with AM, of the angular-momentum matrix too). centroidal_kernel (taskspace_kernels.hip) and the
// whole-body instantiation of ik_kernel (ik_kernels.hip) call these, so jac_com is the same bits in both.
// Included after step_kernels.hip (small math) and dyn_kernels.hip (DynTab).
#pragma once

namespace mjl {

// lane = subtree root s: the mass ms and centre of mass c of the bodies [s, send), xim[k] = (xipos_k, mass_k).
// A massless subtree (`empty`): c = xi, the root's own xipos, and inv = 0.
static INL void cent_subtree_com(const float (*xim)[4], int s, int send, const float* xi, float* c, float& ms,
                                 float& inv, bool& empty) {
  ms = 0.f;
  float sum[3] = {0.f, 0.f, 0.f};
  for (int k = s; k < send; k++) {
    const float mk = xim[k][3];
    ms += mk;
    for (int i = 0; i < 3; i++) sum[i] += mk * xim[k][i];
  }
  empty = ms < kMinVal;
  inv = empty ? 0.f : 1.f / ms;
  for (int i = 0; i < 3; i++) c[i] = empty ? xi[i] : sum[i] * inv;
}

// the bodies of S(bs) that dof d (of body db) moves: all of it (bs), the subtree of the dof's body (db), or none (-1)
static INL int cent_moved_set(const DynTab* tab, int bs, int d, int db, const int* ssend, bool isd) {
  int S = -1;
  if (isd) {
    if ((tab->body_dofmask[bs] >> d) & 1u) S = bs;
    else if (db > bs && db < ssend[bs]) S = db;
  }
  return S;
}

// Column d of jac_com (jc) and, with AM, of angmom_mat (am) of the subtree rooted at bs, S = cent_moved_set's set:
// closed form on that set's composite. cm[k] = (centre of mass, mass) and cI[k] the inertia about it, per subtree.
template <bool AM>
static INL void cent_column(int S, int bs, const float (*cm)[4], const float (*cI)[6], int kind, const float* ax,
                            const float* an, float* jc, float* am) {
  const float mb = cm[bs][3];
  for (int i = 0; i < 3; i++) jc[i] = 0.f;
  if constexpr (AM)
    for (int i = 0; i < 3; i++) am[i] = 0.f;
  if (S >= 0 && mb > 0.f) {
    const float mS = cm[S][3], k = mS / mb;
    const float cS[3] = {cm[S][0], cm[S][1], cm[S][2]};
    float t[3] = {ax[0], ax[1], ax[2]};  // the velocity of the set's centre of mass per unit rate
    if (kind == 0) {
      const float r[3] = {cS[0] - an[0], cS[1] - an[1], cS[2] - an[2]};
      t[0] = t[1] = t[2] = 0.f;
      add_cross(t, ax, r);
      if constexpr (AM) {
        const float* I = cI[S];
        am[0] = I[0] * ax[0] + I[3] * ax[1] + I[4] * ax[2];
        am[1] = I[3] * ax[0] + I[1] * ax[1] + I[5] * ax[2];
        am[2] = I[4] * ax[0] + I[5] * ax[1] + I[2] * ax[2];
      }
    }
    if constexpr (AM) {
      const float dc[3] = {cS[0] - cm[bs][0], cS[1] - cm[bs][1], cS[2] - cm[bs][2]};
      const float mt[3] = {mS * t[0], mS * t[1], mS * t[2]};
      add_cross(am, dc, mt);
    }
    for (int i = 0; i < 3; i++) jc[i] = k * t[i];
  }
}

}  // namespace mjl

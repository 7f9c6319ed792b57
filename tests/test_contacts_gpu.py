"""Contact readout on the GPU (mjx.forward_contacts / mjl_forward_contacts) against the CPU oracle's
contact list and constraint forces, and against the forward pass's own outputs.

States: every keyframe plus 24 random states from default_rng(0) per model (the recipe of
tests/test_gpu_parity.py). Tolerances are that file's (fp32 kernel vs fp64 oracle): 2e-5 absolute for
dist / pos / frame, 2e-3 * (1 + max|ref| of the env) for forces. Counts, geoms, dims and row addresses
are exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import _lib, abi, mjx
from mjx_amd._header import HEADER
from oracle import Oracle, state_arrays

pytestmark = pytest.mark.gpu

FIELDS = ("ncon", "geom", "dim", "efc_address", "dist", "pos", "frame", "force", "body_force")


def _states(m, n_random=24, seed=0):
    rng = np.random.default_rng(seed)
    od = Oracle(m)
    out = [(m.key_qpos[k].copy(), np.zeros(m.nv), np.zeros(m.nv), rng.uniform(-1, 1, m.nu)) for k in range(m.nkey)]
    for _ in range(n_random):
        q = m.qpos0.copy()
        q[7:] += rng.uniform(-0.3, 0.3, m.nq - 7)
        q[2] += rng.uniform(-0.25, 0.05)
        s = od.new_state(q, rng.uniform(-1, 1, m.nv), ctrl=rng.uniform(-1, 1, m.nu))
        nst = int(rng.integers(0, 60))
        if nst:
            od.rollout(s, rng.uniform(-1, 1, (nst, m.nu)))
        a = state_arrays(m, s)
        out.append((a["qpos"], a["qvel"], a["qacc_warmstart"], rng.uniform(-1, 1, m.nu)))
    return [tuple(np.float32(x).astype(np.float64) for x in st) for st in out]


def _load(sys_, states, nenv=None):
    """A batch holding the states (tiled to nenv envs when given)."""
    nenv = len(states) if nenv is None else nenv
    d = mjx.make_data(sys_, nenv)
    idx = np.arange(nenv) % len(states)
    for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
        d.set(f, torch.tensor(np.array([s[i] for s in states])[idx], dtype=torch.float32))
    return d


def _np(c):
    return {f: None if getattr(c, f) is None else getattr(c, f).cpu().numpy() for f in FIELDS}


def _all_fields(d):
    return {f: d.get(f).cpu().numpy() for f in abi.FIELD}


@pytest.fixture(scope="module", params=["humanoid_mjx", "humanoid"])
def setup(request):
    """Model, states, the oracle's forward pass of each state, and ONE full readout (max_con = ncon_max,
    body forces on) with the batch it ran on; shared by the tests, which leave all of it unchanged."""
    m = mjx_amd.load_model(request.param)
    sys_ = mjx.put_model(m)
    states = _states(m)
    orc = Oracle(m)
    ref = [state_arrays(m, orc.forward(orc.new_state(*st))) for st in states]
    d = _load(sys_, states)
    full = _np(mjx.forward_contacts(sys_, d, body_force=True))
    return m, sys_, states, ref, full, _all_fields(d)


def _match(g_geom, g_pos, o_geom, o_pos):
    """GPU contact -> oracle contact: same (geom1, geom2), the nearest position where a pair has two.
    Each oracle contact is taken once; returns the permutation (or fails)."""
    used, perm = set(), []
    for c in range(len(g_geom)):
        cand = [j for j in range(len(o_geom)) if j not in used and tuple(o_geom[j]) == tuple(g_geom[c])]
        assert cand, f"GPU contact {c} {tuple(g_geom[c])} has no oracle contact left"
        j = min(cand, key=lambda j: np.abs(o_pos[j] - g_pos[c]).max())
        used.add(j)
        perm.append(j)
    assert used == set(range(len(o_geom))), "an oracle contact has no GPU contact"
    return perm


def _oracle_contact_forces(m, a):
    """Per oracle contact: (dim, first row, contact-frame force) from efc_force / efc_type: the contact rows
    follow the limit rows (types 0 / 1); a type-2 contact has one row, a type-3 (pyramidal) one four,
    +t1, -t1, +t2, -t2."""
    pair = {(int(g1), int(g2)): p for p, (g1, g2) in enumerate(zip(m.pair_geom1, m.pair_geom2))}
    typ, f = a["efc_type"], a["efc_force"]
    adr = int((typ < 2).sum())
    out = []
    for j in range(a["ncon"]):
        mu = m.pair_friction[pair[tuple(int(x) for x in a["con_geom"][j])]][0]
        if typ[adr] == 2:
            out.append((1, adr, np.array([f[adr], 0.0, 0.0])))
            adr += 1
        else:
            assert typ[adr] == 3
            r = f[adr:adr + 4]
            out.append((3, adr, np.array([r.sum(), (r[0] - r[1]) * mu, (r[2] - r[3]) * mu])))
            adr += 4
    assert adr == a["nefc"]
    return out


def test_parity_with_oracle(setup):
    m, sys_, states, ref, G, _ = setup
    nshared = nbodybody = 0
    kinds = set()
    for i, a in enumerate(ref):
        n = a["ncon"]
        assert G["ncon"][i] == n, f"state {i}: ncon"
        perm = _match(G["geom"][i, :n], G["pos"][i, :n], a["con_geom"], a["con_pos"])
        ocf = _oracle_contact_forces(m, a)
        s = 1.0 + (np.abs(a["efc_force"]).max() if a["nefc"] else 0.0)
        nlim = int((a["efc_type"] < 2).sum())
        adr = nlim
        for c, j in enumerate(perm):
            what = f"state {i} contact {c} (oracle {j})"
            assert abs(G["dist"][i, c] - a["con_dist"][j]) <= 2e-5, what
            np.testing.assert_allclose(G["pos"][i, c], a["con_pos"][j], rtol=0, atol=2e-5, err_msg=what)
            for r in range(3):
                np.testing.assert_allclose(G["frame"][i, c, r], a["con_frame"][j][3 * r:3 * r + 3], rtol=0, atol=2e-5,
                                           err_msg=f"{what} frame row {r}")
            dim, _, fo = ocf[j]
            assert G["dim"][i, c] == dim, what
            err = np.abs(G["force"][i, c] - fo).max()
            assert err <= 2e-3 * s, f"{what} force: err {err:.3e} > 2e-3 * {s:.3g}"
            # rows in contact order: the first contact's row follows the limit rows, steps 1 or 4 by dim
            assert G["efc_address"][i, c] == adr, what
            adr += 1 if G["dim"][i, c] == 1 else 4
            kinds.add(dim)
        assert adr == a["nefc"], f"state {i}: rows"
        pairs = [tuple(g) for g in G["geom"][i, :n]]
        nshared += sum(pairs.count(p) > 1 for p in pairs)
        nbodybody += sum(m.geom_bodyid[g1] != 0 and m.geom_bodyid[g2] != 0 for g1, g2 in pairs)
    # the states exercise what the readout has to get right
    assert max(a["ncon"] for a in ref) == 8 and min(a["ncon"] for a in ref) == 0
    assert nshared > 0 and nbodybody > 0 and kinds == {1, 3}


def test_body_forces_sum_to_the_roots_constraint_force(setup):
    """One tree with a free root: the root's translational qfrc_constraint is the sum of every contact force
    on the tree's bodies (limit rows and body-body contacts cancel), and the world body takes the opposite."""
    m, sys_, states, ref, G, F = setup
    fw = mjx.forward_contacts(sys_, _load(sys_, states)).force_world().cpu().numpy().astype(np.float64)
    assert fw.shape == G["force"].shape
    body = np.asarray(m.geom_bodyid)
    for i in range(len(states)):
        q = F["qfrc_constraint"][i].astype(np.float64)
        tol = 2e-3 * (1 + np.abs(q).max())
        bf = G["body_force"][i].astype(np.float64)
        assert np.abs(bf[1:].sum(0) - q[:3]).max() <= tol, f"state {i}: sum over bodies"
        assert np.abs(-bf[0] - q[:3]).max() <= tol, f"state {i}: world body"
        tot = np.zeros(3)
        for c in range(G["ncon"][i]):  # force_world() summed the same way
            g1, g2 = G["geom"][i, c]
            tot += fw[i, c] * (float(body[g2] != 0) - float(body[g1] != 0))
        assert np.abs(tot - q[:3]).max() <= tol, f"state {i}: force_world"


def test_same_forward_and_option_untouched(setup):
    m, sys_, states, ref, G, F = setup
    d = _load(sys_, states)
    mjx.forward(sys_, d)
    plain = _all_fields(d)
    for f in abi.FIELD:
        np.testing.assert_array_equal(F[f], plain[f], err_msg=f)
    # the batch's own option still decides later calls, and both settings give these same fields
    d2 = _load(sys_, states)
    for force in (0, 1):
        d2.set_option(abi.OPT_FORCE_GLOBAL_ROWS, force)
        mjx.forward_contacts(sys_, d2, max_con=1)
        for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
            d2.set(f, torch.tensor(np.array([s[i] for s in states]), dtype=torch.float32))
        mjx.forward(sys_, d2)
        after = _all_fields(d2)
        for f in abi.FIELD:
            np.testing.assert_array_equal(after[f], plain[f], err_msg=f"{f} (option {force})")


def test_capacity(setup):
    m, sys_, states, ref, G, _ = setup
    assert G["geom"].shape[1] == sys_.ncon_max
    small = _np(mjx.forward_contacts(sys_, _load(sys_, states), max_con=3, body_force=True))
    np.testing.assert_array_equal(small["ncon"], G["ncon"])
    assert small["ncon"].max() == 8
    for f in FIELDS[1:-1]:
        assert small[f].shape[:2] == (len(states), 3)
        np.testing.assert_array_equal(small[f], G[f][:, :3], err_msg=f)
    np.testing.assert_array_equal(small["body_force"], G["body_force"])
    for i, n in enumerate(G["ncon"]):  # the sentinel past ncon
        assert (G["geom"][i, n:] == -1).all() and (G["geom"][i, :n] >= 0).all()
        for f in FIELDS[2:-1]:
            assert not G[f][i, n:].any(), f"state {i} {f}"


def _raw_call(sys_, d, mask, mc, marker):
    """mjl_forward_contacts into marker-filled buffers of the caller's."""
    n, dev = d.nenv, d.device
    I = lambda *s: torch.full(s, int(marker), dtype=torch.int32, device=dev)
    Fl = lambda *s: torch.full(s, float(marker), dtype=torch.float32, device=dev)
    out = dict(ncon=I(n), geom=I(n, mc, 2), dim=I(n, mc), efc_address=I(n, mc), dist=Fl(n, mc), pos=Fl(n, mc, 3),
               frame=Fl(n, mc, 3, 3), force=Fl(n, mc, 3), body_force=Fl(n, sys_.nbody, 3))
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().mjl_forward_contacts(d.handle, None if mask is None else p(mask), mc,
                                               *[p(out[f]) for f in FIELDS], None))
    return {f: t.cpu().numpy() for f, t in out.items()}


def test_mask_and_batch_edges(setup):
    m, sys_, states, ref, G, _ = setup
    B, ns, mc = 67, len(states), sys_.ncon_max
    mask = (torch.arange(B, device="cuda") % 2 == 0).float()
    on = mask.cpu().numpy() > 0.5
    got = _raw_call(sys_, _load(sys_, states, B), mask, mc, -7)
    idx = np.arange(B) % ns
    for f in FIELDS:
        np.testing.assert_array_equal(got[f][on], G[f][idx][on], err_msg=f)
        assert (got[f][~on] == -7).all(), f"{f}: a masked-out row was written"
    # the Python front end defines the masked-out rows: the sentinel
    c = _np(mjx.forward_contacts(sys_, _load(sys_, states, B), mask=mask, body_force=True))
    assert (c["geom"][~on] == -1).all() and not c["ncon"][~on].any() and not c["frame"][~on].any()
    np.testing.assert_array_equal(c["force"][on], G["force"][idx][on])
    # every output but ncon may be NULL
    d = _load(sys_, states, B)
    ncon = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    _lib.check(L.mjl_forward_contacts(d.handle, None, 1, C.c_void_p(ncon.data_ptr()), *([None] * 9)))
    np.testing.assert_array_equal(ncon.cpu().numpy(), G["ncon"][idx])
    err = HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_forward_contacts(d.handle, None, 1, *([None] * 10)) == err  # ncon is required
    assert L.mjl_forward_contacts(d.handle, None, 0, C.c_void_p(ncon.data_ptr()), *([None] * 9)) == err


def test_graph_capture_replays_on_new_states(setup):
    m, sys_, states, ref, G, _ = setup
    ns = len(states)
    other = [states[(i + 5) % ns] for i in range(ns)]
    d = _load(sys_, states)
    mjx.forward_contacts(sys_, d, body_force=True)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = mjx.forward_contacts(sys_, d, body_force=True)
    for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
        d.set(f, torch.tensor(np.array([st[i] for st in other]), dtype=torch.float32))
    g.replay()
    torch.cuda.synchronize()
    got = _np(c)
    perm = (np.arange(ns) + 5) % ns
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], G[f][perm], err_msg=f)

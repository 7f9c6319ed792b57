"""Static evidence from a gfx950 assembly listing (`make -C mujoco-mjx-lab_amd/csrc asm`, /tmp/mjx355.s):

* the Newton loop of the speed-test kernel = the strongly connected component of the kernel's machine
  CFG (basic blocks = labels, edges = branches and fall-through) that holds the most
  v_mfma_f32_32x32x2 instructions (the Hessian's and the factor's): instruction counts by class;
* VGPRs, SGPR / VGPR spills, scratch and LDS of every step_kernel / APG instantiation, from the
  listing's kernel metadata.

  python tools/newton_loop_stats.py /tmp/mjx355.s [kernel-name-substring ...]
"""
import re
import sys
from collections import Counter


def kernels(path):
    """{name: [instruction or label lines]} of every function in the listing."""
    out, name, body = {}, None, []
    for ln in open(path, errors="replace"):
        s = ln.strip()
        m = re.match(r"^([A-Za-z_][\w.$]*):", s)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            out[name] = body
            continue
        if s.startswith(".Lfunc_end"):
            name = None
        if name is None or not s or s.startswith((";", ".")) and not s.startswith(".LBB"):
            continue
        body.append(s.split(";")[0].strip())
    return out


def blocks(body):
    """Basic blocks [(label, [instr])] and successor lists by block index."""
    bl, cur = [], ("entry", [])
    for s in body:
        m = re.match(r"^(\.LBB[\w.]*):", s)
        if m:
            bl.append(cur)
            cur = (m.group(1), [])
        elif s:
            cur[1].append(s)
    bl.append(cur)
    idx = {b[0]: i for i, b in enumerate(bl)}
    succ = []
    for i, (_, ins) in enumerate(bl):
        t, fall = [], True
        for k, s in enumerate(ins):
            op = s.split()[0]
            if op.startswith("s_cbranch") or op == "s_branch":
                tgt = s.split()[-1]
                if tgt in idx:
                    t.append(idx[tgt])
                if op == "s_branch" and k == len(ins) - 1:
                    fall = False
            if op in ("s_endpgm", "s_setpc_b64") and k == len(ins) - 1:
                fall = False
        if fall and i + 1 < len(bl):
            t.append(i + 1)
        succ.append(t)
    return bl, succ


def sccs(succ):
    n, index, low, on, st, out, cnt = len(succ), {}, {}, set(), [], [], [0]
    for root in range(n):
        if root in index:
            continue
        work = [(root, 0)]
        while work:
            v, pi = work.pop()
            if pi == 0:
                index[v] = low[v] = cnt[0]
                cnt[0] += 1
                st.append(v)
                on.add(v)
            rec = False
            for k in range(pi, len(succ[v])):
                w = succ[v][k]
                if w not in index:
                    work.append((v, k + 1))
                    work.append((w, 0))
                    rec = True
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            if rec:
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = st.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                out.append(comp)
            if work:
                p = work[-1][0]
                low[p] = min(low[p], low[v])
    return out


def classify(ins):
    c = Counter()
    for s in ins:
        op = s.split()[0]
        c["total"] += 1
        if op.startswith("s_"):
            c["scalar"] += 1
        if op.startswith("v_mov"):
            c["v_mov"] += 1
        if re.match(r"v_(fma|fmac)_", op):
            c["fma/fmac"] += 1
        if op.startswith("v_readlane"):
            c["readlane"] += 1
        if op == "s_and_saveexec_b64":
            c["s_and_saveexec_b64"] += 1
        if op in ("s_cbranch_execz", "s_cbranch_execnz"):
            c["cbranch_exec"] += 1
        if re.match(r"s_(and|or|xor|andn2|orn2|not|mov|cselect)_b64$", op):
            c["64-bit mask ops"] += 1
        if op.startswith("v_cndmask"):
            c["v_cndmask"] += 1
        if op.startswith("ds_read"):
            c["ds_read*"] += 1
        if op.startswith("ds_write"):
            c["ds_write*"] += 1
        if op == "s_waitcnt" and "lgkmcnt" in s:
            c["s_waitcnt lgkmcnt"] += 1
        if op == "s_barrier":
            c["s_barrier"] += 1
        if op.startswith("v_mfma"):
            c["mfma"] += 1
    return c


def resources(path, pats):
    """Per-kernel metadata from the listing's amdhsa.kernels block."""
    txt = open(path, errors="replace").read()
    rows = []
    for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
        blk = ".agpr_count:" + blk
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
        name = g("name")
        if any(p in name for p in pats):
            rows.append((name, g("vgpr_count"), g("agpr_count"), g("sgpr_count"), g("sgpr_spill_count"),
                         g("vgpr_spill_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size")))
    return rows


def main():
    path = sys.argv[1]
    pats = sys.argv[2:] or ["step_kernel", "apg", "vjp"]
    ks = kernels(path)
    for name, body in ks.items():
        m = re.search(r"step_kernelINS_4DimsI.*?EEELi(\d+)ELi\d+EEE", name)
        if not m or m.group(1) not in ("2", "3"):  # MODE_SPEEDTEST = 2, MODE_ENV_STEP = 3
            continue
        bl, succ = blocks(body)
        best, bestn = None, 0
        for comp in sccs(succ):
            if len(comp) < 2:
                continue
            ins = [s for i in comp for s in bl[i][1]]
            n = sum(1 for s in ins if s.startswith("v_mfma_f32_32x32x2"))
            if n > bestn:
                best, bestn = ins, n
        whole = sum(len(b[1]) for b in bl)
        if best is None:
            print(f"{name}: no loop with 32x32x2 MFMAs; whole kernel {whole}")
            continue
        c = classify(best)
        print(f"{name}\n  Newton loop (SCC) " + ", ".join(f"{k} {v}" for k, v in c.items()) + f"; whole kernel {whole}")
    print("kernel: vgpr agpr sgpr sgpr_spill vgpr_spill scratch_bytes lds_bytes")
    for r in resources(path, pats):
        print("  " + r[0] + ": " + " ".join(r[1:]))


if __name__ == "__main__":
    main()

"""Plain references for the device-resident dogleg's aux row (k_bw_aux) and first linearisation (k_bw_solve_step, phases P1 - P6), in
numpy longdouble (docs/device_solve_pins.md).

Every function takes the SAME fp64 numbers the device read — parameter blocks, the pre-integrations' numbers including sqrt_info, the
prior's matrices, the folded lidar moments — as a dict of arrays (`inputs`), plus the integer layout of the problem (`meta`), and returns
(values, M): per compared array the reference values and, entry by entry, the sum of the absolute values of the terms of the entry's last
contraction.  `with_unit` turns that into the comparison unit

    u[e] = max( max over 32 draws | R(inputs o (1 +- 2^-52)) - R(inputs) |[e] ,  eps64 M[e] )

and the tests assert |Q - R| <= 16 u entrywise (GPU) and <= 4 u (the product's one-thread replay on the CPU).  A structural zero has
M = 0 and no draw moves it: u = 0, the comparison is exact.

The IMU block is written from the factor's mathematics as oracle/imu.h states it (residual of the mid-point pre-integration corrected to
first order in the biases; Jacobians in the tangent [dp, dtheta] of a pose with q <- q * [1, dtheta / 2]); the lidar linear maps and the
extrinsic prior go through the oracle's factor functions (an independent Jacobian in fp64); the rest is index arithmetic.
Quaternions are (w, x, y, z) inside, (x, y, z, w) in a pose's last four entries, and are used as they come: nothing renormalises an input.
"""
import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
DRAWS = 32
GPU_MARGIN, CPU_MARGIN = 16.0, 4.0


def ld(a):
    return np.asarray(a, dtype=LD)


# ------------------------------------------------------------------------------------------------ small algebra
def skew(v):
    z = LD(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=LD)


def q_of_pose(p):
    return ld([p[6], p[3], p[4], p[5]])


def qmul(a, b):
    return ld([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
               a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def qconj(q):
    return ld([q[0], -q[1], -q[2], -q[3]])


def qinv(q):
    return qconj(q) / (q @ q)


def rotm(q):
    """the rotation q v q^-1 of a unit quaternion as a polynomial in its entries (no normalisation)"""
    w, x, y, z = q
    one, two = LD(1), LD(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=LD)


def delta_q(theta):
    return ld([LD(1), theta[0] / 2, theta[1] / 2, theta[2] / 2])


def left3(q):
    return np.eye(3, dtype=LD) * q[0] + skew(q[1:])


def left4(q):
    m = np.zeros((4, 4), LD)
    m[:3, :3] = left3(q)
    m[3, :3], m[:3, 3], m[3, 3] = -q[1:], q[1:], q[0]
    return m


def right4(q):
    m = np.zeros((4, 4), LD)
    m[:3, :3] = np.eye(3, dtype=LD) * q[0] - skew(q[1:])
    m[3, :3], m[:3, 3], m[3, 3] = -q[1:], q[1:], q[0]
    return m


# ------------------------------------------------------------------------------------------------ IMU block
O_P, O_R, O_V, O_BA, O_BG = 0, 3, 6, 9, 12


def imu_raw(pm, pose_i, sb_i, pose_j, sb_j, wrong=None):
    """unwhitened residual (15) and Jacobian (15 x 30, tangent columns pose_i 6 | sb_i 9 | pose_j 6 | sb_j 9).
    wrong: None, or a deliberate mistake for the tests that show the comparison catches one ('sign', 'zero_block')."""
    pose_i, sb_i, pose_j, sb_j = ld(pose_i), ld(sb_i), ld(pose_j), ld(sb_j)
    dp, dq, dv, ba, bg, g = ld(pm["dp"]), ld(pm["dq"]), ld(pm["dv"]), ld(pm["ba"]), ld(pm["bg"]), ld(pm["g"])
    T, Jb = ld(pm["sum_dt"]), ld(pm["jac"])
    Pi, Qi, Pj, Qj = pose_i[:3], q_of_pose(pose_i), pose_j[:3], q_of_pose(pose_j)
    Vi, Bai, Bgi = sb_i[0:3], sb_i[3:6], sb_i[6:9]
    Vj, Baj, Bgj = sb_j[0:3], sb_j[3:6], sb_j[6:9]
    dp_dba, dp_dbg = Jb[O_P:O_P + 3, O_BA:O_BA + 3], Jb[O_P:O_P + 3, O_BG:O_BG + 3]
    dq_dbg = Jb[O_R:O_R + 3, O_BG:O_BG + 3]
    dv_dba, dv_dbg = Jb[O_V:O_V + 3, O_BA:O_BA + 3], Jb[O_V:O_V + 3, O_BG:O_BG + 3]
    dba, dbg = Bai - ba, Bgi - bg
    cq = qmul(dq, delta_q(dq_dbg @ dbg))
    cv = dv + dv_dba @ dba + dv_dbg @ dbg
    cp = dp + dp_dba @ dba + dp_dbg @ dbg
    Qii = qinv(Qi)
    RiT = rotm(Qii)
    half = LD(1) / 2
    a_p = RiT @ (-half * g * T * T + Pj - Pi - Vi * T)
    a_v = RiT @ (-g * T + Vj - Vi)
    r = np.zeros(15, LD)
    r[O_P:O_P + 3] = a_p - cp
    r[O_R:O_R + 3] = 2 * qmul(qinv(cq), qmul(Qii, Qj))[1:]
    r[O_V:O_V + 3] = a_v - cv
    r[O_BA:O_BA + 3] = Baj - Bai
    r[O_BG:O_BG + 3] = Bgj - Bgi
    J = np.zeros((15, 30), LD)
    I3 = np.eye(3, dtype=LD)
    # pose_i
    J[O_P:O_P + 3, 0:3] = -RiT
    J[O_P:O_P + 3, 3:6] = skew(a_p)
    J[O_R:O_R + 3, 3:6] = -(left4(qmul(qinv(Qj), Qi)) @ right4(cq))[:3, :3]
    J[O_V:O_V + 3, 3:6] = skew(a_v)
    # speed-bias i
    c = 6
    J[O_P:O_P + 3, c + 0:c + 3] = -RiT * T
    J[O_P:O_P + 3, c + 3:c + 6] = -dp_dba
    J[O_P:O_P + 3, c + 6:c + 9] = -dp_dbg
    J[O_R:O_R + 3, c + 6:c + 9] = -left3(qmul(qmul(qinv(Qj), Qi), cq)) @ dq_dbg
    J[O_V:O_V + 3, c + 0:c + 3] = -RiT
    J[O_V:O_V + 3, c + 3:c + 6] = -dv_dba
    J[O_V:O_V + 3, c + 6:c + 9] = -dv_dbg
    J[O_BA:O_BA + 3, c + 3:c + 6] = -I3
    J[O_BG:O_BG + 3, c + 6:c + 9] = -I3
    # pose_j
    c = 15
    J[O_P:O_P + 3, c + 0:c + 3] = RiT
    J[O_R:O_R + 3, c + 3:c + 6] = left3(qmul(qmul(qinv(cq), Qii), Qj))
    # speed-bias j
    c = 21
    J[O_V:O_V + 3, c + 0:c + 3] = RiT
    J[O_BA:O_BA + 3, c + 3:c + 6] = I3
    J[O_BG:O_BG + 3, c + 6:c + 9] = I3
    if wrong == "sign":
        J[O_V:O_V + 3, 3:6] = -J[O_V:O_V + 3, 3:6]
    elif wrong == "zero_block":
        J[O_R:O_R + 3, 18:21] = 0
    elif wrong is not None:
        raise ValueError(wrong)
    return r, J


def imu_block(pm, pose_i, sb_i, pose_j, sb_j, wrong=None):
    """-> (out (932): J^T J 30 x 30 | J^T r 30 | cost | 1, M (932)) of the factor whitened by the upper triangle of sqrt_info"""
    r, J = imu_raw(pm, pose_i, sb_i, pose_j, sb_j, wrong)
    S = np.triu(ld(pm["sqrt_info"]))
    Jw, rw = S @ J, S @ r
    out, M = np.zeros(932, LD), np.zeros(932, LD)
    out[:900] = (Jw.T @ Jw).ravel()
    out[900:930] = Jw.T @ rw
    out[930] = (rw @ rw) / 2
    out[931] = 1
    aJ, ar = np.abs(Jw), np.abs(rw)
    M[:900] = (aJ.T @ aJ).ravel()
    M[900:930] = aJ.T @ ar
    M[930] = (ar @ ar) / 2
    return out, M


# ------------------------------------------------------------------------------------------------ lidar linear map (through the oracle)
def lidar_map(oracle, pose_p, pose_i, pose_ex):
    """L (18 x 13) and l (13) with j = L z, r = l^T z, z = [w0 (p, 1), w1 (p, 1), w2 (p, 1), d]: the factor is linear in the plane
    normal and affine in the point, so column 4 a + b is the factor's Jacobian at (normal e_a, point e_b) minus the one at (e_a, 0)
    for b < 3 and the one at (e_a, 0) for b = 3; d moves no Jacobian and adds itself to the residual.  -> (out (247), M (247))"""
    pp, pi, pe = (np.asarray(v, np.float64) for v in (pose_p, pose_i, pose_ex))
    out, M = np.zeros(247, LD), np.zeros(247, LD)
    L, ML = out[:234].reshape(18, 13), M[:234].reshape(18, 13)
    for a in range(3):
        coeff = np.zeros(4)
        coeff[a] = 1.0
        probes = []
        for b in range(4):
            p = np.zeros(3)
            if b:
                p[b - 1] = 1.0
            res, js = oracle.factor_ppp(p, coeff, pp, pi, pe)
            probes.append((ld(np.concatenate([js[0][:6], js[1][:6], js[2][:6]])), LD(res)))
        j0, r0 = probes[0]
        for b in range(3):
            L[:, 4 * a + b] = probes[b + 1][0] - j0
            ML[:, 4 * a + b] = np.abs(probes[b + 1][0]) + np.abs(j0)
            out[234 + 4 * a + b] = probes[b + 1][1] - r0
            M[234 + 4 * a + b] = abs(probes[b + 1][1]) + abs(r0)
        L[:, 4 * a + 3] = j0
        ML[:, 4 * a + 3] = np.abs(j0)
        out[234 + 4 * a + 3] = r0
        M[234 + 4 * a + 3] = abs(r0)
    out[246] = 1
    return out, M


# ------------------------------------------------------------------------------------------------ priors, relative poses
def prior_dx(meta, inp):
    x0 = ld(inp["prior_x0"])
    dx = np.zeros(meta["n_prior"], LD)
    for kind, index, size, off, x0_off in meta["keep"]:
        xv = ld(inp["pose"][index] if kind == 0 else (inp["sb"][index] if kind == 1 else inp["ex"]))
        b0 = x0[x0_off:x0_off + size]
        if size != 7:
            dx[off:off + size] = xv - b0
        else:
            dx[off:off + 3] = xv[:3] - b0[:3]
            dq = qmul(qinv(q_of_pose(b0)), q_of_pose(xv))
            v = 2 * (dq / np.sqrt(dq @ dq))[1:]
            dx[off + 3:off + 6] = -v if dq[0] < 0 else v
    return dx


def prior_row(meta, inp):
    """-> (out (np + 1): Jtr0 + JtJ dx | 0.5 |lin_res + lin_jac dx|^2, M)"""
    n = meta["n_prior"]
    dx = prior_dx(meta, inp)
    JtJ, lin_jac, lin_res, Jtr0 = ld(inp["prior_JtJ"]), ld(inp["prior_lin_jac"]), ld(inp["prior_lin_res"]), ld(inp["prior_Jtr0"])
    out, M = np.zeros(n + 1, LD), np.zeros(n + 1, LD)
    out[:n] = Jtr0 + JtJ @ dx
    M[:n] = np.abs(Jtr0) + np.abs(JtJ) @ np.abs(dx)
    rr = lin_res + lin_jac @ dx
    out[n] = (rr @ rr) / 2
    M[n] = out[n]
    return out, M


def exprior_row(oracle, inp):
    """the extrinsic PriorFactor through the oracle -> (out (43): J^T J 6 x 6 | J^T r 6 | cost, M)"""
    rot = np.asarray(inp["ex_prior_rot"], np.float64)
    r, J = oracle.factor_prior(np.asarray(inp["ex_prior_pos"], np.float64), np.array([rot[1], rot[2], rot[3], rot[0]]), np.asarray(inp["ex"], np.float64))
    r, J = ld(r), ld(J)[:, :6]
    out, M = np.zeros(43, LD), np.zeros(43, LD)
    out[:36] = (J.T @ J).ravel()
    out[36:42] = J.T @ r
    out[42] = (r @ r) / 2
    M[:36] = (np.abs(J).T @ np.abs(J)).ravel()
    M[36:42] = np.abs(J).T @ np.abs(r)
    M[42] = out[42]
    return out, M


def relative_poses(meta, inp):
    """T_{pivot<-i} of the lidar frames from the body poses and the extrinsic -> (out (Wo, 12): R row-major | t, M)"""
    Wo = meta["Wo"]
    out, M = np.zeros((Wo, 12), LD), np.zeros((Wo, 12), LD)
    ex = ld(inp["ex"])
    tlb, qlb = ex[:3], q_of_pose(ex)
    pp = ld(inp["pose"][0])
    Qlp = qmul(q_of_pose(pp), qconj(qlb))
    Plp_a, Plp_b = pp[:3], rotm(Qlp) @ tlb
    for i in range(Wo):
        pi = ld(inp["pose"][i + 1])
        Qli = qmul(q_of_pose(pi), qconj(qlb))
        Pli_b = rotm(Qli) @ tlb
        R = rotm(qmul(qconj(Qlp), Qli))
        RT = rotm(qconj(Qlp))
        d = (pi[:3] - Pli_b) - (Plp_a - Plp_b)
        out[i, :9], out[i, 9:] = R.ravel(), RT @ d
        M[i, :9] = 1
        M[i, 9:] = np.abs(RT) @ (np.abs(pi[:3]) + np.abs(Pli_b) + np.abs(Plp_a) + np.abs(Plp_b))
    return out, M


# ------------------------------------------------------------------------------------------------ the aux row and the assembly
def aux_row(meta, inp, oracle, wrong=None):
    """everything k_bw_aux writes for one window at the parameters of `inp` (+ cand_Rt, which launch B writes from the same parameters)
    -> (dict of arrays, dict of M)"""
    Wo = meta["Wo"]
    v, m = {}, {}
    v["imu_out"], m["imu_out"] = np.zeros((Wo, 932), LD), np.zeros((Wo, 932), LD)
    v["lmap"], m["lmap"] = np.zeros((Wo, 247), LD), np.zeros((Wo, 247), LD)
    for i in range(Wo):
        if meta["present"][i]:
            v["imu_out"][i], m["imu_out"][i] = imu_block(inp["pim"][i], inp["pose"][i], inp["sb"][i], inp["pose"][i + 1], inp["sb"][i + 1], wrong)
        v["lmap"][i], m["lmap"][i] = lidar_map(oracle, inp["pose"][0], inp["pose"][i + 1], inp["ex"])
    if meta["have_prior"]:
        v["prior_out"], m["prior_out"] = prior_row(meta, inp)
    if meta["use_ex_prior"]:
        v["exprior_out"], m["exprior_out"] = exprior_row(oracle, inp)
    v["cand_Rt"], m["cand_Rt"] = relative_poses(meta, inp)
    return v, m


def frame_rows(meta, f):
    """global tangent rows of lidar frame f + 1's 18 local ones: pose_0 | pose_{f+1} | extrinsic (-1: the extrinsic is constant)"""
    exc = meta["ex_col"]
    return np.array(list(range(6)) + list(range(15 * (f + 1), 15 * (f + 1) + 6)) + [exc + k if exc >= 0 else -1 for k in range(6)])


def assemble(meta, inp, oracle):
    """The normal equations at the parameters of `inp` with the moments inp['S'] (Wo x 258), in the order prior, IMU factors, lidar
    frames, extrinsic prior; then Jacobi-scaled by inp['scale'] (a scale fixed earlier), or by 1 / (1 + sqrt(diag H)) of this very H.
    -> (dict H (n x n) g (n) scale (n) costs (4: marg, pim, ppp, extrinsic prior), dict of M)"""
    Wo, n = meta["Wo"], meta["n"]
    aux, am = aux_row(meta, inp, oracle)
    H, g, MH, Mg = np.zeros((n, n), LD), np.zeros(n, LD), np.zeros((n, n), LD), np.zeros(n, LD)
    costs, Mc = np.zeros(4, LD), np.zeros(4, LD)
    if meta["have_prior"]:
        pc = np.asarray(meta["prior_col"][:n])
        on = np.flatnonzero(pc >= 0)
        JtJ = ld(inp["prior_JtJ"])
        H[np.ix_(on, on)] += JtJ[np.ix_(pc[on], pc[on])]
        MH[np.ix_(on, on)] += np.abs(JtJ[np.ix_(pc[on], pc[on])])
        g[on] += aux["prior_out"][pc[on]]
        Mg[on] += am["prior_out"][pc[on]]
        costs[0], Mc[0] = aux["prior_out"][-1], am["prior_out"][-1]
    for i in range(Wo):
        if not meta["present"][i]:
            continue
        o, mo = aux["imu_out"][i], am["imu_out"][i]
        sl = slice(15 * i, 15 * i + 30)
        H[sl, sl] += o[:900].reshape(30, 30)
        MH[sl, sl] += mo[:900].reshape(30, 30)
        g[sl] += o[900:930]
        Mg[sl] += mo[900:930]
        costs[1] += o[930]
        Mc[1] += mo[930]
    S = ld(inp["S"])
    for f in range(Wo):
        costs[2] += S[f, 256]
        Mc[2] += abs(S[f, 256])
        if S[f, 257] == 0:
            continue
        L, l = aux["lmap"][f][:234].reshape(18, 13), aux["lmap"][f][234:247]
        Sf = S[f, :256].reshape(16, 16)[:13, :13]
        LS = L @ Sf
        Hb, gb = LS @ L.T, LS @ l
        MHb, Mgb = np.abs(LS) @ np.abs(L).T, np.abs(LS) @ np.abs(l)
        rows = frame_rows(meta, f)
        on = np.flatnonzero(rows >= 0)
        H[np.ix_(rows[on], rows[on])] += Hb[np.ix_(on, on)]
        MH[np.ix_(rows[on], rows[on])] += MHb[np.ix_(on, on)]
        g[rows[on]] += gb[on]
        Mg[rows[on]] += Mgb[on]
    exc = meta["ex_col"]
    if meta["use_ex_prior"]:
        costs[3], Mc[3] = aux["exprior_out"][42], am["exprior_out"][42]
        if exc >= 0:
            sl = slice(exc, exc + 6)
            H[sl, sl] += aux["exprior_out"][:36].reshape(6, 6)
            MH[sl, sl] += am["exprior_out"][:36].reshape(6, 6)
            g[sl] += aux["exprior_out"][36:42]
            Mg[sl] += am["exprior_out"][36:42]
    s = ld(inp["scale"]) if "scale" in inp else 1 / (1 + np.sqrt(np.diag(H)))
    ss = np.outer(s, s)
    v = dict(H=H * ss, g=g * s, scale=s, costs=costs, H_unscaled=H, g_unscaled=g)
    m = dict(H=MH * ss, g=Mg * s, scale=s, costs=Mc, H_unscaled=MH, g_unscaled=Mg)
    return v, m


# ------------------------------------------------------------------------------------------------ the unit of the comparisons
FLOAT_KEYS = ("pose", "sb", "ex", "prior_x0", "prior_JtJ", "prior_lin_jac", "prior_lin_res", "prior_Jtr0", "ex_prior_pos", "ex_prior_rot", "S", "scale")
PIM_KEYS = ("dp", "dq", "dv", "ba", "bg", "g", "sum_dt", "jac", "sqrt_info")


def perturbed(inp, rng):
    """every fp64 input times (1 + 2^-52) or (1 - 2^-52), the sign drawn per number; in longdouble, nothing renormalised"""
    def one(a):
        a = ld(a)
        return a * (1 + LD(2.0 ** -52) * ld(rng.choice([-1.0, 1.0], size=a.shape)))
    out = {k: one(inp[k]) for k in FLOAT_KEYS if k in inp}
    if "pim" in inp:
        out["pim"] = [None if p is None else {k: one(p[k]) for k in PIM_KEYS} for p in inp["pim"]]
    return out


def with_unit(fn, inp, seed=0, draws=DRAWS):
    """fn(inputs) -> (dict of arrays, dict of M).  -> (values at inp, unit u per array)"""
    base, M = fn(inp)
    dev = {k: np.zeros(np.shape(v), LD) for k, v in base.items()}
    rng = np.random.default_rng(seed)
    for _ in range(draws):
        got, _m = fn(perturbed(inp, rng))
        for k in dev:
            dev[k] = np.maximum(dev[k], np.abs(got[k] - base[k]))
    unit = {k: np.maximum(dev[k], EPS64 * np.abs(M[k])) for k in dev}
    return base, unit


def ratio(got, ref, unit):
    """max over the entries of |got - ref| / u; an entry with u = 0 must be equal (ratio 0) or counts as infinitely far"""
    d = np.abs(ld(got) - ref)
    r = np.where(unit > 0, d / np.where(unit > 0, unit, 1), np.where(d == 0, 0, np.inf))
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ inputs from the hook's dict
def meta_of(lin):
    return dict(Wo=lin["Wo"], n=lin["n"], ex_col=lin["ex_col"], n_prior=lin["n_prior"], have_prior=lin["have_prior"], use_ex_prior=lin["use_ex_prior"],
                keep=[tuple(int(v) for v in row) for row in lin["keep"]], prior_col=np.asarray(lin["prior_col"]), present=[int(v) for v in lin["present"]])


def inputs_of(lin, point, S=None, scale=None):
    """point: 'x' or 'cand' — the parameters the reference is evaluated at"""
    P = lin[point]
    inp = dict(pose=P["pose"], sb=P["sb"], ex=P["ex"], prior_x0=lin["prior_x0"], ex_prior_pos=lin["ex_prior_pos"], ex_prior_rot=lin["ex_prior_rot"],
               prior_JtJ=lin["prior"]["JtJ"], prior_lin_jac=lin["prior"]["lin_jac"], prior_lin_res=lin["prior"]["lin_res"], prior_Jtr0=lin["prior"]["Jtr0"],
               pim=[pm if lin["present"][i] else None for i, pm in enumerate(lin["pim"])])
    if S is not None:
        inp["S"] = S
    if scale is not None:
        inp["scale"] = scale
    return inp

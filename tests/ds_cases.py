"""Synthetic problems for tests/ds_ref.py in the shape lio_est_batch_get_linearization returns (capi.EstimatorBatch.linearization), built on
the CPU from the oracle's pre-integration, and the text exchange with tests/host/aux_row_check.hip.

A case is a dict like the hook's: Wo, n, ex_col, n_prior, have_prior, use_ex_prior, keep, prior_col, present, pim (dp, dq as w x y z, dv,
ba, bg, g, sum_dt, jac, sqrt_info = chol(inv(cov))^T), prior matrices, x (pose, sb, ex), plus S (Wo x 258 moments) and `cov` per
pre-integration for the conditioning the formula check measures."""
import numpy as np

from lio_amd import capi

G_NORM = 9.805


def _quat_mul(a, b):   # x y z w
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _small_q(rng, s):
    v = rng.normal(0, s, 3) / 2
    q = np.array([v[0], v[1], v[2], 1.0])
    return q / np.linalg.norm(q)


def make_pim(oracle, rng, ba, bg, samples=40, dt=0.005):
    acc0 = np.array([0.3, 0.0, 9.8]) + rng.normal(0, 0.2, 3)
    gyr0 = np.array([0.0, 0.0, 0.2]) + rng.normal(0, 0.05, 3)
    pim = capi.Pim(oracle, acc0, gyr0, ba, bg, acc_n=0.2, gyr_n=0.02, acc_w=0.0002, gyr_w=2.0e-5, g_norm=G_NORM)
    for k in range(samples):
        pim.push_back(dt, np.array([0.3 + 0.2 * np.sin(0.1 * k), 0.0, 9.8]) + rng.normal(0, 0.05, 3),
                      np.array([0.0, 0.0, 0.2 + 0.05 * np.cos(0.07 * k)]) + rng.normal(0, 0.01, 3))
    d = pim.get()
    L = np.linalg.cholesky(np.linalg.inv(d["cov"]))
    q = d["dq"]
    num = dict(dp=d["dp"].copy(), dq=np.array([q[3], q[0], q[1], q[2]]), dv=d["dv"].copy(), ba=np.array(ba, float), bg=np.array(bg, float),
               g=np.array([0.0, 0.0, -G_NORM]), sum_dt=float(d["sum_dt"]), jac=d["jac"].copy(), sqrt_info=np.ascontiguousarray(L.T), cov=d["cov"].copy())
    return pim, num


def make_case(oracle, Wo, ex_free, have_prior, use_ex_prior, seed, empty_frame=-1, flip_block=-1, state_noise=1.0):
    """one window: Wo + 1 states chained through Wo pre-integrations (each factor nearly satisfied, plus noise), a prior over
    (pose_0 .. pose_{Wo-1}, sb_0, extrinsic) linearised near the states, an extrinsic prior, lidar moments of a few hundred residuals per
    frame.  empty_frame: a frame without residuals.  flip_block: the kept pose whose x0 quaternion is negated (dq.w < 0 in the prior)."""
    rng = np.random.default_rng(seed)
    F = Wo + 1
    pose, sb = np.zeros((F, 7)), np.zeros((F, 9))
    q0 = np.array([0.02, -0.01, 0.3, 0.0])
    q0[3] = np.sqrt(1 - q0[:3] @ q0[:3])
    pose[0] = np.r_[[1.0, 2.0, 0.5], q0]
    sb[0] = [1.5, 0.3, 0.0, 0.01, -0.02, 0.015, 0.001, -0.002, 0.0015]
    pims, handles = [], []
    g = np.array([0.0, 0.0, -G_NORM])
    for f in range(1, F):
        h, num = make_pim(oracle, rng, sb[f - 1][3:6], sb[f - 1][6:9])
        handles.append(h)
        pims.append(num)
        T = num["sum_dt"]
        R = _rot(pose[f - 1][3:])
        dq = num["dq"]
        qj = _quat_mul(pose[f - 1][3:], np.array([dq[1], dq[2], dq[3], dq[0]]))
        qj = _quat_mul(qj, _small_q(rng, 2e-3 * state_noise))
        pose[f] = np.r_[pose[f - 1][:3] + sb[f - 1][:3] * T + 0.5 * g * T * T + R @ num["dp"] + rng.normal(0, 3e-3 * state_noise, 3), qj / np.linalg.norm(qj)]
        sb[f] = np.r_[sb[f - 1][:3] + g * T + R @ num["dv"] + rng.normal(0, 3e-3 * state_noise, 3), sb[f - 1][3:6] + rng.normal(0, 1e-4, 3),
                      sb[f - 1][6:9] + rng.normal(0, 1e-5, 3)]
    ex = np.r_[[0.05, -0.02, -0.08], _small_q(rng, 0.03)]
    n = 15 * F + (6 if ex_free else 0)
    case = dict(Wo=Wo, n=n, ex_col=15 * F if ex_free else -1, have_prior=int(have_prior), use_ex_prior=int(use_ex_prior), present=np.ones(Wo, np.int32),
                pim=pims, x=dict(pose=pose, sb=sb, ex=ex), pim_handles=handles)
    case["ex_prior_pos"] = ex[:3] + rng.normal(0, 1e-3, 3)
    qp = _quat_mul(ex[3:], _small_q(rng, 0.01))
    case["ex_prior_rot"] = np.array([qp[3], qp[0], qp[1], qp[2]])
    # the prior: kept blocks pose_0 .. pose_{Wo-1} | speed-bias 0 | extrinsic
    keep, x0 = [], []
    off = xo = 0
    for i in range(Wo):
        keep.append((0, i, 7, off, xo)); off += 6; xo += 7
        b = np.r_[pose[i][:3] + rng.normal(0, 5e-3, 3), _quat_mul(pose[i][3:], _small_q(rng, 4e-3))]
        if i == flip_block:
            b[3:] = -b[3:]
        x0.append(b)
    keep.append((1, 0, 9, off, xo)); off += 9; xo += 9
    x0.append(sb[0] + rng.normal(0, 1e-3, 9))
    keep.append((2, 0, 7, off, xo)); off += 6; xo += 7
    x0.append(np.r_[ex[:3] + rng.normal(0, 1e-3, 3), _quat_mul(ex[3:], _small_q(rng, 2e-3))])
    npr = off
    prior_col = -np.ones(n, np.int32)
    if have_prior:
        for kind, index, size, o, _ in keep:
            col = 15 * index if kind == 0 else (15 * index + 6 if kind == 1 else case["ex_col"])
            if col >= 0:
                prior_col[col:col + (6 if size == 7 else size)] = np.arange(o, o + (6 if size == 7 else size))
    lin_jac = rng.normal(0, 1, (npr, npr)) * np.exp(rng.uniform(-1, 5, npr))[None, :]
    lin_res = rng.normal(0, 0.5, npr)
    px0 = np.zeros(90)
    flat = np.concatenate(x0)
    px0[:flat.size] = flat
    case.update(n_prior=npr if have_prior else 0, n_keep=len(keep) if have_prior else 0, keep=np.array(keep if have_prior else np.zeros((0, 5)), np.int32).reshape(-1, 5),
                prior_col=prior_col, prior_x0=px0 if have_prior else np.zeros(90))
    m = npr if have_prior else 0
    case["prior"] = dict(JtJ=(lin_jac.T @ lin_jac)[:m, :m].copy(), lin_jac=lin_jac[:m, :m].copy(), lin_res=lin_res[:m].copy(),
                         Jtr0=(lin_jac.T @ lin_res)[:m].copy())
    # lidar moments: S = sum rho' z z^T over random residuals
    S = np.zeros((Wo, 258))
    for f in range(Wo):
        if f == empty_frame:
            continue
        K = 300 + 37 * f
        w = rng.normal(0, 1, (K, 3))
        w[::3] = np.c_[rng.normal(0, 0.05, (len(w[::3]), 2)), np.ones(len(w[::3]))]
        w /= np.linalg.norm(w, axis=1)[:, None]
        p = rng.normal(0, 1, (K, 3)) * [15, 15, 2]
        r = rng.normal(0, 0.05, K)
        d = r - np.einsum("ij,ij->i", w, p)
        z = np.zeros((K, 16))
        for a in range(3):
            z[:, 4 * a:4 * a + 3] = w[:, a:a + 1] * p
            z[:, 4 * a + 3] = w[:, a]
        z[:, 12] = d
        rho = 1.0 / (1.0 + r * r)
        S[f, :256] = ((z * rho[:, None]).T @ z).ravel()
        S[f, 256] = 0.5 * np.sum(np.log1p(r * r))
        S[f, 257] = K
    case["S"] = S
    return case


def _num(vals):
    return " ".join(float(v).hex() for v in np.asarray(vals, np.float64).ravel())


def write_cases(path, cases):
    """the text input of tests/host/aux_row_check.hip: integers in decimal, doubles as C99 hex floats (exact)"""
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for c in cases:
            Wo, n, npr = c["Wo"], c["n"], c["n_prior"]
            f.write(f"{Wo} {n} {c['ex_col']} {npr} {c['have_prior']} {c['use_ex_prior']} {c['n_keep']}\n")
            f.write(" ".join(str(int(v)) for v in np.asarray(c["keep"]).ravel()) + "\n")
            f.write(" ".join(str(int(v)) for v in c["prior_col"]) + "\n")
            f.write(" ".join(str(int(v)) for v in c["present"]) + "\n")
            f.write(_num(c["x"]["pose"]) + "\n" + _num(c["x"]["sb"]) + "\n" + _num(c["x"]["ex"]) + "\n")
            f.write(_num(c["prior_x0"]) + "\n" + _num(c["ex_prior_pos"]) + "\n" + _num(c["ex_prior_rot"]) + "\n")
            for pm in c["pim"]:
                f.write(_num(np.concatenate([pm["dp"], pm["dq"], pm["dv"], pm["ba"], pm["bg"], pm["g"], [pm["sum_dt"]], pm["jac"].ravel(), pm["sqrt_info"].ravel()])) + "\n")
            pr = c["prior"]
            f.write(_num(np.concatenate([pr["JtJ"].ravel(), pr["lin_jac"].ravel(), pr["lin_res"], pr["Jtr0"], [0.0]])) + "\n")
            f.write(_num(c["S"]) + "\n")


def read_results(path, cases):
    """what the program wrote, per case: imu_out, lmap, prior_out, exprior_out, cand_Rt (the aux row at x), then the first
    linearisation of solve_step with max_iterations = 0: scale, g, Hcur (n x n), costs0 and (it, termination, done, need_host)"""
    tok = open(path).read().split()
    pos = 0

    def take(k, shape=None):
        nonlocal pos
        a = np.array([float.fromhex(t) for t in tok[pos:pos + k]])
        pos += k
        return a.reshape(shape) if shape else a

    out = []
    for c in cases:
        Wo, n, npr = c["Wo"], c["n"], c["n_prior"]
        r = dict(imu_out=take(Wo * 932, (Wo, 932)), lmap=take(Wo * 248, (Wo, 248)), prior_out=take(npr + 1), exprior_out=take(44), cand_Rt=take(Wo * 12, (Wo, 12)),
                 scale=take(n), g=take(n), Hcur=take(n * n, (n, n)), costs0=take(4))
        r["it"], r["termination"], r["done"], r["need_host"] = (int(v) for v in take(4))
        out.append(r)
    assert pos == len(tok)
    return out


def standard_cases(oracle):
    """Wo in {2, 5, 7} x (extrinsic free / constant) x (prior / none) x (extrinsic prior / none), a frame without residuals, a kept pose
    whose prior quaternion has the other sign"""
    return [
        make_case(oracle, 2, False, False, False, 11),
        make_case(oracle, 2, True, True, True, 12, flip_block=1),
        make_case(oracle, 2, False, True, True, 13, empty_frame=0),
        make_case(oracle, 5, True, True, False, 14, empty_frame=2),
        make_case(oracle, 5, False, True, True, 15, flip_block=0),
        make_case(oracle, 7, False, True, True, 16),
        make_case(oracle, 7, True, True, True, 17, empty_frame=6),
        make_case(oracle, 2, True, False, True, 18, state_noise=10.0),
    ]

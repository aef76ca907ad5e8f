/*
 * orc_models.inc -- the Model plugins of the reference (include/acrobot.h, include/double_integrator.h) and
 * the synthetic LQ model, written once for an arithmetic type MT and included by ilqr_oracle.c
 *   - as MT = orc_real (names as written): what the rollouts integrate,
 *   - and, in the fp32 build only, again as MT = orc_fd = double (names suffixed _fd): what the
 *     finite-difference sweep differentiates.  eps = 1e-3 second differences of a cost of O(1e3) are
 *     rounding noise in float (1e3 * 6e-8 / 4e-6 = 15 against Hessian entries of 800), so the fp32 mode
 *     of the product evaluates ITS finite differences in double from the float knot and stores the
 *     records as float; this twin does the same.  In the fp64 / fp80 builds both flavours are one.
 * TEST INFRASTRUCTURE ONLY (see ilqr_oracle.h).
 */
/* include/acrobot.h:43-81.  Parameters I1=I2=l1=l2=m1=m2=1, lc1=lc2=0.5, g=9.81 (:19-25). */
static void MN(acrobot_dynamics)(const orc_model* m, const MT* x, const MT* u, MT* dx) {
  (void)m;
  const MT I1 = 1, I2 = 1, l1 = 1, l2 = 1, m1 = 1, m2 = 1, g = 9.81;
  const MT lc1 = (MT)0.5 * l1, lc2 = (MT)0.5 * l2;
  const MT q0 = x[0], q1 = x[1], qd0 = x[2], qd1 = x[3];
  /* H(q), acrobot.h:43-51 */
  const MT c2 = cos(q1);
  const MT H00 = I1 + I2 + m2 * l1 * l1 + 2 * m2 * l1 * lc2 * c2;
  const MT H01 = I2 + m2 * l1 * lc2 * c2;
  const MT H10 = I2 + m2 * l1 * lc2 * c2;
  const MT H11 = I2;
  /* C(q,qdot), acrobot.h:53-61 */
  const MT s2 = sin(q1);
  const MT C00 = -2 * m2 * l1 * lc2 * s2 * qd1;
  const MT C01 = -m2 * l2 * lc2 * s2 * qd1;
  const MT C10 = m2 * l1 * lc2 * s2 * qd0;
  const MT C11 = 0;
  /* G(q), acrobot.h:63-70 */
  const MT s1 = sin(q0);
  const MT s1p2 = sin(q0 + q1);
  const MT G0 = m1 * g * lc1 * s1 + m2 * g * (l1 * s1 + lc2 * s1p2);
  const MT G1 = m2 * g * lc2 * s1p2;
  /* rhs = (0,u) - C*qdot - G, acrobot.h:80 */
  const MT Cq0 = C00 * qd0 + C01 * qd1;
  const MT Cq1 = C10 * qd0 + C11 * qd1;
  const MT r0 = ((MT)0.0 - Cq0) - G0;
  const MT r1 = (u[0] - Cq1) - G1;
  /* H.inverse() for a fixed 2x2: Eigen LU/InverseImpl.h:76-96 (invdet = 1/det; 4 products) */
  const MT det = H00 * H11 - H10 * H01;
  const MT invdet = (MT)1.0 / det;
  const MT Hi00 = H11 * invdet;
  const MT Hi10 = -H10 * invdet;
  const MT Hi01 = -H01 * invdet;
  const MT Hi11 = H00 * invdet;
  dx[0] = qd0; /* acrobot.h:79 */
  dx[1] = qd1;
  dx[2] = Hi00 * r0 + Hi01 * r1;
  dx[3] = Hi10 * r0 + Hi11 * r1;
}

/* include/acrobot.h:83-92: Ks=Kd=0, Kr=0.1 */
static MT MN(acrobot_cost)(const orc_model* m, const MT* x, const MT* u) {
  const MT q0 = m->goal[0] - x[0], q1 = m->goal[1] - x[1];
  const MT qd0 = m->goal[2] - x[2], qd1 = m->goal[3] - x[3];
  const MT Ks = 0.0, Kd = 0.0, Kr = 0.1;
  return Ks * Ks * (q0 * q0 + q1 * q1) + Kd * Kd * (qd0 * qd0 + qd1 * qd1) + Kr * Kr * (u[0] * u[0]);
}

/* include/acrobot.h:94-100: Ks=Kd=20 */
static MT MN(acrobot_final_cost)(const orc_model* m, const MT* x) {
  const MT q0 = m->goal[0] - x[0], q1 = m->goal[1] - x[1];
  const MT qd0 = m->goal[2] - x[2], qd1 = m->goal[3] - x[3];
  const MT Ks = 20.0, Kd = 20.0;
  return Ks * Ks * (q0 * q0 + q1 * q1) + Kd * Kd * (qd0 * qd0 + qd1 * qd1);
}


/* include/double_integrator.h:29-37, mass = 1 (:51) */
static void MN(dint_dynamics)(const orc_model* m, const MT* x, const MT* u, MT* dx) {
  (void)m;
  const MT mass = 1.0;
  dx[0] = x[2];
  dx[1] = x[3];
  dx[2] = u[0] / mass;
  dx[3] = u[1] / mass;
}
static const MT MN(DINT_HX)[4] = {1, 1, 0.2, 0.2}; /* double_integrator.h:19-22 (diagonal) */
/* double_integrator.h:39-43: (goal-x)' Hx (goal-x) + u' Hu u, Hu = I.  Evaluated as
 * (d' Hx) d with the dense 4x4 Hx; the off-diagonal zeros contribute exact +0 terms. */
static MT MN(dint_quad4)(const MT* goal, const MT* x, MT scale) {
  /* (d' H) d for the dense 4x4 H: row_j = d_j*H_jj (+ exact zeros); the final dot of two
   * dynamic 4-vectors is reduced by Eigen's SSE2 redux as (r0 d0 + r2 d2) + (r1 d1 + r3 d3)
   * (Core/Redux.h linear vectorised traversal, two packet accumulators). */
  MT r[4], d[4];
  for (int i = 0; i < 4; i++) {
    d[i] = goal[i] - x[i];
    r[i] = scale * (MN(DINT_HX)[i] * d[i]); /* gemv applies the extracted scalar factor last */
  }
  return (r[0] * d[0] + r[2] * d[2]) + (r[1] * d[1] + r[3] * d[3]);
}
static MT MN(dint_cost)(const orc_model* m, const MT* x, const MT* u) {
  MT goal[4];
  for (int i = 0; i < 4; i++) goal[i] = m->goal[i];
  const MT cx = MN(dint_quad4)(goal, x, 1.0);
  const MT cu = (u[0] * (MT)1.0) * u[0] + (u[1] * (MT)1.0) * u[1];
  return cx + cu;
}
/* double_integrator.h:45-48: (goal-x)' (10 Hx) (goal-x) */
static MT MN(dint_final_cost)(const orc_model* m, const MT* x) {
  MT goal[4];
  for (int i = 0; i < 4; i++) goal[i] = m->goal[i];
  return MN(dint_quad4)(goal, x, 10.0);
}

/* Synthetic LQ model (BASELINE.json configs[4]; no counterpart in the reference, SURVEY.md 0.1):
 * xdot = A x + B u (row-major A[nx][nx], B[nx][nu]); cost 0.5 (x'Qx + u'Ru) [+ x'N u when N is set]; final 0.5 x'Qf x.
 * Sums run left to right over the column index. */
static void MN(lq_dynamics)(const orc_model* m, const MT* x, const MT* u, MT* dx) {
  const int n = m->nx, mu = m->nu;
  for (int i = 0; i < n; i++) {
    MT a = 0;
    for (int j = 0; j < n; j++) a += m->A[i * n + j] * x[j];
    for (int j = 0; j < mu; j++) a += m->Bm[i * mu + j] * u[j];
    dx[i] = a;
  }
}
static MT MN(lq_quad)(int n, const orc_real* M, const MT* v) {
  MT s = 0;
  for (int i = 0; i < n; i++) {
    MT r = 0;
    for (int j = 0; j < n; j++) r += M[i * n + j] * v[j];
    s += v[i] * r;
  }
  return s;
}
static MT MN(lq_cost)(const orc_model* m, const MT* x, const MT* u) {
  MT c = (MT)0.5 * (MN(lq_quad)(m->nx, m->Q, x) + MN(lq_quad)(m->nu, m->R, u));
  if (m->N) { /* + x'N u */
    for (int i = 0; i < m->nx; i++) {
      MT r = 0;
      for (int j = 0; j < m->nu; j++) r += m->N[i * m->nu + j] * u[j];
      c += x[i] * r;
    }
  }
  return c;
}
static MT MN(lq_final_cost)(const orc_model* m, const MT* x) {
  return (MT)0.5 * MN(lq_quad)(m->nx, m->Qf, x);
}


/* A chain of N damped pendulums coupled by torsion springs, every second one actuated (nx = 2 N, nu = N / 2): a dense NON-quadratic
 * model for the generic path -- no counterpart among the reference's two shipped models; it is a plugin written against the reference's
 * Model interface (include/model.h:6-21: dynamics / cost / final_cost, public u_min / u_max) the way examples/user_model_pendulum_chain.hpp
 * writes it for the device, term for term.  x = (theta_0 .. theta_{N-1}, omega_0 .. omega_{N-1}); parameters in goal[0..7]:
 * g/l, damping, coupling, w_theta, w_omega, w_u, final scale, target angle. */
static void MN(chain_dynamics)(const orc_model* m, const MT* x, const MT* u, MT* dx) {
  const int N = m->nx / 2;
  const MT gl = m->goal[0], damp = m->goal[1], kc = m->goal[2];
  for (int i = 0; i < N; i++) dx[i] = x[N + i];
  for (int i = 0; i < N; i++) {
    const MT th = x[i];
    MT lap = 0;
    if (i > 0) lap += x[i - 1] - th;
    if (i < N - 1) lap += x[i + 1] - th;
    MT acc = -gl * sin(th);
    acc -= damp * x[N + i];
    acc += kc * lap;
    if ((i & 1) == 0) acc += u[i >> 1];
    dx[N + i] = acc;
  }
}
static MT MN(chain_state_cost)(const orc_model* m, const MT* x) {
  const int N = m->nx / 2;
  const MT wq = m->goal[3], ww = m->goal[4], target = m->goal[7];
  MT s = 0;
  for (int i = 0; i < N; i++) {
    s += wq * ((MT)1.0 - cos(x[i] - target));
    s += ((MT)0.5 * ww) * (x[N + i] * x[N + i]);
  }
  return s;
}
static MT MN(chain_cost)(const orc_model* m, const MT* x, const MT* u) {
  const MT wu = m->goal[5];
  MT s = MN(chain_state_cost)(m, x);
  for (int j = 0; j < m->nu; j++) s += ((MT)0.5 * wu) * (u[j] * u[j]);
  return s;
}
static MT MN(chain_final_cost)(const orc_model* m, const MT* x) {
  const MT wf = m->goal[6];
  return wf * MN(chain_state_cost)(m, x);
}

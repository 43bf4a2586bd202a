// orbx_svd4.inc — the 4x4 DLT solve that Initializer::CheckRT (orbx_checkrt_kernel.hip) and CreateNewMapPoints
// (orbx_match_tri_kernel.hip) share: the right singular vector of the smallest singular value, by one-sided Jacobi in f64 (column
// pairs in (i, j) order, at most 30 sweeps), uncontracted, operation for operation the CPU restatement's.  Included inside
// namespace orbx by the .hip file that uses it.
__device__ void smallestRightSingularVector4(const double Ain[16], double x[4]) {
  double At[4][4], V[4][4], W[4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int k = 0; k < 4; k++) { At[i][k] = Ain[k * 4 + i]; V[i][k] = i == k ? 1.0 : 0.0; }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) sd += At[i][k] * At[i][k];
    W[i] = sd;
  }
  const double eps = 2.2204460492503131e-16 * 10;
  for (int iter = 0; iter < 30; iter++) {
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = i + 1; j < 4; j++) {
        double a = W[i], p = 0, b = W[j];
#pragma unroll
        for (int k = 0; k < 4; k++) p += At[i][k] * At[j][k];
        if (!(fabs(p) <= eps * sqrt(a * b))) {
          p *= 2;
          const double beta = a - b, gamma = sqrt(p * p + beta * beta);
          double c, sn;
          if (beta < 0) {
            const double delta = (gamma - beta) * 0.5;
            sn = sqrt(delta / gamma);
            c = p / (gamma * sn * 2);
          } else {
            c = sqrt((gamma + beta) / (gamma * 2));
            sn = p / (gamma * c * 2);
          }
          a = b = 0;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const double t0 = c * At[i][k] + sn * At[j][k], t1 = -sn * At[i][k] + c * At[j][k];
            At[i][k] = t0; At[j][k] = t1;
            a += t0 * t0; b += t1 * t1;
          }
          W[i] = a; W[j] = b;
          changed = true;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const double t0 = c * V[i][k] + sn * V[j][k], t1 = -sn * V[i][k] + c * V[j][k];
            V[i][k] = t0; V[j][k] = t1;
          }
        }
      }
    if (!changed) break;
  }
  // smallest squared column norm, the first one among equals (selects instead of a dynamic index: the arrays stay in registers)
  double wb = W[0];
#pragma unroll
  for (int k = 0; k < 4; k++) x[k] = V[0][k];
#pragma unroll
  for (int i = 1; i < 4; i++) {
    const bool lt = W[i] < wb;
    wb = lt ? W[i] : wb;
#pragma unroll
    for (int k = 0; k < 4; k++) x[k] = lt ? V[i][k] : x[k];
  }
}

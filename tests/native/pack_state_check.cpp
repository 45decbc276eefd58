// pack_state / unpack_state of host_graph.h against an independent restatement of the device form (tests/test_abi_and_host.py):
//   SE2 x, y, cos, sin | XY x, y, 0, 0 | SE3 t (3), 0 | q (4) / |q|, the norm the square root of qx^2 + qy^2 + qz^2 + qw^2 in that order.
// Everything is compared with ==.  The inputs are read through volatile so that neither side is folded at compile time.
#include <cmath>
#include <cstdio>

#include "host_graph.h"

using namespace rrpgo;

static int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

static const double kPi = 3.14159265358979323846;   // rounds to the double next below pi: inside (-pi, pi]
static volatile double v_theta[] = {0.0, 0.1, -0.1, 1.5707963267948966, -3.0, 3.0, kPi, 2.5e-9, -3.1415926535897922};
static volatile double v_xy[][2] = {{0.0, 0.0}, {1.25, -7.5}, {-1e6, 3e-7}, {0.3, 0.1}};
static volatile double v_t[][3] = {{0.0, 0.0, 0.0}, {1.5, -2.25, 1e3}, {-0.1, 0.2, -0.3}};
static volatile double v_q[][4] = {{0.0, 0.0, 0.0, 1.0},            // the unit
                                   {0.1, -0.2, 0.3, 0.9},           // not of unit length
                                   {0.5, 0.5, 0.5, -0.5},           // negative w
                                   {-3.0, 4.0, 12.0, -84.0},        // far from unit length, negative w
                                   {1e-3, 2e-3, -2e-3, 1e-3}};

static const double kPoison = -123.456;

int main() {
  // ---- SE2
  for (volatile double &vt : v_theta)
    for (volatile double(&vx)[2] : v_xy) {
      const double th = vt, s[3] = {vx[0], vx[1], th};
      double p[8], u[3] = {kPoison, kPoison, kPoison};
      for (double &x : p) x = kPoison;
      CHECK(pack_state(NODE_SE2, s, p) == node_state_len(NODE_SE2));
      CHECK(p[0] == s[0] && p[1] == s[1]);
      CHECK(p[2] == std::cos(th) && p[3] == std::sin(th));
      CHECK(p[4] == 0.0 && p[5] == 0.0 && p[6] == 0.0 && p[7] == 0.0);
      CHECK(unpack_state(NODE_SE2, p, u) == node_state_len(NODE_SE2));
      CHECK(u[0] == s[0] && u[1] == s[1]);
      CHECK(u[2] == std::atan2(std::sin(th), std::cos(th)));   // atan2's own result, bit for bit
      // ... which is theta up to the roundings of cos and sin (each below 2^-53 of the unit vector) and of atan2 (an ulp, at most 2^-51)
      CHECK(std::fabs(u[2] - th) <= 1e-15);
      CHECK(u[2] > -kPi - 1e-15 && u[2] <= kPi);
    }
  {   // theta = pi stays pi (not -pi)
    const double s[3] = {0.0, 0.0, v_theta[6]};
    double p[8], u[3];
    pack_state(NODE_SE2, s, p);
    unpack_state(NODE_SE2, p, u);
    CHECK(u[2] > 3.0);
  }
  // ---- XY
  for (volatile double(&vx)[2] : v_xy) {
    const double s[2] = {vx[0], vx[1]};
    double p[8], u[3] = {kPoison, kPoison, kPoison};
    for (double &x : p) x = kPoison;
    CHECK(pack_state(NODE_XY, s, p) == node_state_len(NODE_XY));
    CHECK(p[0] == s[0] && p[1] == s[1] && p[2] == 0.0 && p[3] == 0.0);
    CHECK(p[4] == 0.0 && p[5] == 0.0 && p[6] == 0.0 && p[7] == 0.0);
    CHECK(unpack_state(NODE_XY, p, u) == node_state_len(NODE_XY));
    CHECK(u[0] == s[0] && u[1] == s[1]);
    CHECK(u[2] == kPoison);   // two scalars written, not three
  }
  // ---- SE3
  for (volatile double(&vt)[3] : v_t)
    for (volatile double(&vq)[4] : v_q) {
      const double s[7] = {vt[0], vt[1], vt[2], vq[0], vq[1], vq[2], vq[3]};
      const double qx = s[3], qy = s[4], qz = s[5], qw = s[6];
      const double n = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
      CHECK(quat_norm(s + 3) == n);
      double p[8], u[8];
      for (double &x : p) x = kPoison;
      for (double &x : u) x = kPoison;
      CHECK(pack_state(NODE_SE3, s, p) == node_state_len(NODE_SE3));
      CHECK(p[0] == s[0] && p[1] == s[1] && p[2] == s[2] && p[3] == 0.0);
      CHECK(p[4] == qx / n && p[5] == qy / n && p[6] == qz / n && p[7] == qw / n);
      CHECK((p[7] < 0.0) == (qw < 0.0));   // the sign of w is kept: no canonical hemisphere
      CHECK(unpack_state(NODE_SE3, p, u) == node_state_len(NODE_SE3));
      CHECK(u[0] == s[0] && u[1] == s[1] && u[2] == s[2]);
      CHECK(u[3] == p[4] && u[4] == p[5] && u[5] == p[6] && u[6] == p[7]);
      CHECK(u[7] == kPoison);   // seven scalars written
    }
  // the edge numbering coincides with the node numbering: a measurement packs like a state
  CHECK((int)EDGE_SE2 == (int)NODE_SE2 && (int)EDGE_SE2_XY == (int)NODE_XY && (int)EDGE_SE3 == (int)NODE_SE3);
  for (int k = 0; k < 3; k++) CHECK(edge_meas_len(k) == node_state_len(k));
  if (g_failed) return 1;
  std::printf("pack and unpack agree with the restated device form\n");
  return 0;
}

// gtsam_sig: stand-in for <gtsam/linear/HessianFactor.h>: the constructors the reference uses
// (geometric_factor.hpp:459-462 binary, :559-560 unary, radar/factor.hpp:185-186 ternary) and the read accessors.  error(x) = 0.5 x'Gx - x'g + 0.5 f.  NOT GTSAM.
#pragma once
#include <gtsam/linear/GaussianFactor.h>

namespace gtsam
{
class HessianFactor : public GaussianFactor
{
public:
  typedef std::shared_ptr<HessianFactor> shared_ptr;
  HessianFactor(Key j, const Matrix & G, const Vector & g, double f) : G_(G), g_(g), f_(f) { keys_ = {j}; }
  HessianFactor(Key j1, Key j2, const Matrix & G11, const Matrix & G12, const Vector & g1, const Matrix & G22, const Vector & g2, double f)
  : G_(G11.rows() + G22.rows(), G11.cols() + G22.cols()), g_(g1.size() + g2.size()), f_(f)
  {
    keys_ = {j1, j2};
    const int n1 = G11.rows(), n2 = G22.rows();
    for (int r = 0; r < n1; ++r) {
      for (int c = 0; c < n1; ++c) G_(r, c) = G11(r, c);
      for (int c = 0; c < n2; ++c) G_(r, n1 + c) = G_(n1 + c, r) = G12(r, c);
      g_(r) = g1(r);
    }
    for (int r = 0; r < n2; ++r) {
      for (int c = 0; c < n2; ++c) G_(n1 + r, n1 + c) = G22(r, c);
      g_(n1 + r) = g2(r);
    }
  }
  HessianFactor(Key j1, Key j2, Key j3, const Matrix & G11, const Matrix & G12, const Matrix & G13, const Vector & g1, const Matrix & G22,
                const Matrix & G23, const Vector & g2, const Matrix & G33, const Vector & g3, double f)
  : G_(G11.rows() + G22.rows() + G33.rows(), G11.rows() + G22.rows() + G33.rows()), g_(G11.rows() + G22.rows() + G33.rows()), f_(f)
  {
    keys_ = {j1, j2, j3};
    const Matrix * upper[3][3] = {{&G11, &G12, &G13}, {nullptr, &G22, &G23}, {nullptr, nullptr, &G33}};
    const Vector * lin[3] = {&g1, &g2, &g3};
    const int off[3] = {0, G11.rows(), G11.rows() + G22.rows()};
    for (int bi = 0; bi < 3; ++bi) {
      for (int bj = bi; bj < 3; ++bj) {
        const Matrix & B = *upper[bi][bj];
        for (int r = 0; r < B.rows(); ++r)
          for (int c = 0; c < B.cols(); ++c) G_(off[bi] + r, off[bj] + c) = G_(off[bj] + c, off[bi] + r) = B(r, c);
      }
      for (int r = 0; r < lin[bi]->size(); ++r) g_(off[bi] + r) = (*lin[bi])(r);
    }
  }
  Matrix information() const override { return G_; }
  Vector linearTerm() const { return g_; }
  double constantTerm() const { return f_; }

private:
  Matrix G_;
  Vector g_;
  double f_;
};
}  // namespace gtsam

// gtsam_sig: stand-in for <gtsam/slam/BetweenFactor.h>: the relative-pose factor odometry::Manager emits
// (odometry/manager.cpp:53).  It carries its keys, measurement and noise model; evaluating it is GTSAM's business, so error()
// and linearize() throw here.  NOT GTSAM.
#pragma once
#include <stdexcept>

#include <gtsam/linear/NoiseModel.h>
#include <gtsam/nonlinear/NonlinearFactor.h>

namespace gtsam
{
template <class VALUE>
class BetweenFactor : public NonlinearFactor
{
public:
  typedef VALUE T;
  typedef std::shared_ptr<BetweenFactor> shared_ptr;
  BetweenFactor(Key key1, Key key2, const VALUE & measured, const SharedNoiseModel & model = nullptr)
  : NonlinearFactor(KeyVector{key1, key2}), measured_(measured), noise_model_(model)
  {
  }
  Key key1() const { return keys_[0]; }
  Key key2() const { return keys_[1]; }
  const VALUE & measured() const { return measured_; }
  const SharedNoiseModel & noiseModel() const { return noise_model_; }
  size_t dim() const override { return noise_model_ ? noise_model_->dim() : 0; }
  double error(const Values &) const override { throw std::runtime_error("gtsam_sig: BetweenFactor::error is not provided"); }
  std::shared_ptr<GaussianFactor> linearize(const Values &) const override { throw std::runtime_error("gtsam_sig: BetweenFactor::linearize is not provided"); }
  NonlinearFactor::shared_ptr clone() const override { return std::make_shared<BetweenFactor>(*this); }

private:
  VALUE measured_;
  SharedNoiseModel noise_model_;
};
}  // namespace gtsam

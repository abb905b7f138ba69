// gtsam_sig: stand-in for <gtsam/linear/NoiseModel.h>: the diagonal model odometry::Manager builds
// (noiseModel::Diagonal::Sigmas, odometry/manager.cpp:47-51).  NOT GTSAM.
#pragma once
#include <memory>

#include <gtsam/base/Vector.h>

namespace gtsam
{
namespace noiseModel
{
class Base
{
public:
  typedef std::shared_ptr<Base> shared_ptr;
  virtual ~Base() = default;
  size_t dim() const { return dim_; }

protected:
  explicit Base(size_t dim) : dim_(dim) {}
  size_t dim_;
};
class Gaussian : public Base
{
public:
  typedef std::shared_ptr<Gaussian> shared_ptr;

protected:
  explicit Gaussian(size_t dim) : Base(dim) {}
};
class Diagonal : public Gaussian
{
public:
  typedef std::shared_ptr<Diagonal> shared_ptr;
  static shared_ptr Sigmas(const Vector & sigmas, bool smart = true)
  {
    (void)smart;
    return shared_ptr(new Diagonal(sigmas));
  }
  const Vector & sigmas() const { return sigmas_; }
  double sigma(size_t i) const { return sigmas_(static_cast<int>(i)); }

protected:
  explicit Diagonal(const Vector & sigmas) : Gaussian(static_cast<size_t>(sigmas.size())), sigmas_(sigmas) {}
  Vector sigmas_;
};
}  // namespace noiseModel
typedef noiseModel::Base::shared_ptr SharedNoiseModel;
}  // namespace gtsam

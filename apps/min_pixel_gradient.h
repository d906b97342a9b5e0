// --min-pixel-gradient <g>[,<g>...] of both apps (--method semidense): the one parser and the one rule by which the
// command line goes over the configuration file's `min_pixel_gradient (at each level)`.
#ifndef PHOVO_APPS_MIN_PIXEL_GRADIENT_H
#define PHOVO_APPS_MIN_PIXEL_GRADIENT_H

#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "phovo_hip.h"

namespace phovo_apps {

// "<g>[,<g>...]": every value finite and >= 0, at most PHOVO_MAX_LEVELS of them.
inline bool parseMinPixelGradient(const std::string &text, std::vector<double> &out)
{
  out.clear();
  size_t pos = 0;
  while (pos <= text.size()) {
    const size_t comma = text.find(',', pos);
    const std::string item = text.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
    char *end = nullptr;
    const double v = std::strtod(item.c_str(), &end);
    if (item.empty() || *end != '\0' || !std::isfinite(v) || v < 0.0) return false;
    out.push_back(v);
    if (comma == std::string::npos) break;
    pos = comma + 1;
  }
  return !out.empty() && out.size() <= (size_t)PHOVO_MAX_LEVELS;
}

// The command line's thresholds over `opt` (the file's): one value for all levels, or one per level and 0 beyond them.
inline void overrideMinPixelGradient(const std::vector<double> &given, phovo_semidense_options &opt)
{
  if (given.empty()) return;
  for (int l = 0; l < PHOVO_MAX_LEVELS; l++)
    opt.min_pixel_gradient[l] = given.size() == 1 ? given[0] : (size_t)l < given.size() ? given[(size_t)l] : 0.0;
}

// SetSemiDenseOptions() of the class that has it; the other classes have no such options and nothing happens.
template <class Odometry>
auto applyMinPixelGradient(Odometry &odometry, const std::vector<double> &given, int)
    -> decltype(odometry.GetSemiDenseOptions(), void())
{
  phovo_semidense_options opt = odometry.GetSemiDenseOptions();
  overrideMinPixelGradient(given, opt);
  odometry.SetSemiDenseOptions(opt);
}
template <class Odometry>
void applyMinPixelGradient(Odometry &, const std::vector<double> &, long) {}

}  // namespace phovo_apps
#endif

// ref_driver.cpp -- extern "C" surface over the reference's own compiled headers.  TEST INFRASTRUCTURE ONLY.
//
// oracle/Makefile.ref compiles this file against the reference tree (-I $(PHOVO_REFERENCE_DIR)/phovo/include, never
// copied) and the stand-in headers under oracle/ref_standins/ into oracle/_ref/libphovo_ref.so.  What runs behind these
// entry points is the reference's text for eigenPose, warpImage, ComputeResidualsAndJacobians, TestTerminationCriteria and
// Optimize of the Analytic and BiObjective classes; what it runs on (matrix products, the 6x6 inverse, the pyramid
// filters) is ours and documented in the stand-ins.  The Ceres class is not included: it needs Ceres itself.
//
// Iteration counts.  The reference keeps m_Iteration private and overwrites it per level.  The Eigen stand-in calls
// norm_hook at the start of every norm(), which TestTerminationCriteria evaluates once per pass of the loop, and the
// reference's headers are included below with `private` spelt `public` (this translation unit only, standard and stand-in
// headers included before the switch), so the hook reads m_OptimizationLevel and m_Iteration where the reference tests
// them.  The same access lets phovo_ref_analytic_optimize_levels hand prebuilt level planes to Optimize, a test hook that
// therefore stays out of product code.
//
// static_cast<int>(round(x)) on a non-finite or huge x is undefined in C++; on x86-64 the conversion yields INT_MIN, which
// fails the reference's bounds test, the behaviour the oracle states explicitly.
#include <cstdint>
#include <cstring>
#include <exception>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "eigen3/Eigen/Dense"
#include "opencv2/imgproc/imgproc.hpp"
#include "opencv2/highgui/highgui.hpp"
#include "opencv2/contrib/contrib.hpp"

namespace phovo_ref_standin
{
thread_local void (*norm_hook)(void *) = 0;
thread_local void *norm_hook_context = 0;
thread_local std::map< std::string, std::vector< double > > settings;
void unsupported( const char * what ) { throw std::runtime_error( what ); }
}

#define private public
#include "CPhotoconsistencyOdometryAnalytic.h"
#include "CPhotoconsistencyOdometryBiObjective.h"
#undef private

namespace
{
typedef phovo::Analytic::CPhotoconsistencyOdometryAnalytic< unsigned char, double >    AnalyticType;
typedef phovo::Analytic::CPhotoconsistencyOdometryBiObjective< unsigned char, double > BiObjectiveType;

template< class TAligner >
struct IterationProbe
{
  const TAligner * aligner;
  int * iterations_per_level;
  static void hook( void * p )
  {
    IterationProbe * self = static_cast< IterationProbe * >( p );
    const int level = self->aligner->m_OptimizationLevel;
    if( self->iterations_per_level && level >= 0 && level < PHOVO_ORACLE_MAX_LEVELS )
      self->iterations_per_level[ level ] = self->aligner->m_Iteration;
  }
};

void publish_settings( const phovo_oracle_config * cfg )
{
  std::map< std::string, std::vector< double > > & s = phovo_ref_standin::settings;
  s.clear();
  const int n = cfg->num_levels;
  s[ "numOptimizationLevels" ] = std::vector< double >( 1, n );
  s[ "blurFilterSize (at each level)" ] = std::vector< double >( cfg->blur_filter_size, cfg->blur_filter_size + n );
  s[ "imageGradientsScalingFactor (at each level)" ] =
      std::vector< double >( cfg->image_gradients_scaling_factor, cfg->image_gradients_scaling_factor + n );
  s[ "lambda_optimization_step (at each level)" ] =
      std::vector< double >( cfg->lambda_optimization_step, cfg->lambda_optimization_step + n );
  s[ "max_num_iterations (at each level)" ] = std::vector< double >( cfg->max_num_iterations, cfg->max_num_iterations + n );
  s[ "min_gradient_norm (at each level)" ] = std::vector< double >( cfg->min_gradient_norm, cfg->min_gradient_norm + n );
  s[ "visualizeIterations" ] = std::vector< double >( 1, 0.0 );
}

template< class TAligner >
void configure( TAligner & aligner, const phovo_oracle_config * cfg, const double k[9] )
{
  publish_settings( cfg );
  aligner.ReadConfigurationFile( "settings of the driver" );
  aligner.SetMinDepth( cfg->min_depth );
  aligner.SetMaxDepth( cfg->max_depth );
  typename TAligner::Matrix33Type intrinsics;
  for( int i = 0; i < 3; i++ )
    for( int j = 0; j < 3; j++ )
      intrinsics( i, j ) = k[ 3 * i + j ];
  aligner.SetIntrinsicMatrix( intrinsics );
}

template< class TAligner >
void run( TAligner & aligner, double state[6], double rt[16], int * iterations_per_level )
{
  typename TAligner::Vector6Type initial;
  for( int i = 0; i < 6; i++ ) initial( i ) = state[i];
  aligner.SetInitialStateVector( initial );

  IterationProbe< TAligner > probe = { &aligner, iterations_per_level };
  phovo_ref_standin::norm_hook_context = &probe;
  phovo_ref_standin::norm_hook = &IterationProbe< TAligner >::hook;
  try { aligner.Optimize(); }
  catch( ... ) { phovo_ref_standin::norm_hook = 0; throw; }
  phovo_ref_standin::norm_hook = 0;

  const typename TAligner::Vector6Type optimum = aligner.GetOptimalStateVector();
  for( int i = 0; i < 6; i++ ) state[i] = optimum( i );
  const typename TAligner::Matrix44Type pose = aligner.GetOptimalRigidTransformationMatrix();
  if( rt )
    for( int i = 0; i < 4; i++ )
      for( int j = 0; j < 4; j++ )
        rt[ 4 * i + j ] = pose( i, j );
}

template< class TBody >
int guarded( TBody body )
{
  try { body(); return 0; }
  catch( const std::exception & e ) { std::cerr << "phovo_ref: " << e.what() << std::endl; return -1; }
  catch( ... ) { return -2; }
}
} // namespace

extern "C"
{

// SetSourceFrame + SetTargetFrame + Optimize of the Analytic class.  state: initial on entry, optimum on return.
// depth1 may be NULL (the class reads only its type).  iterations_per_level: m_Iteration at the end of each level.
int phovo_ref_analytic_align( const phovo_oracle_config * cfg, const double k[9], int w, int h,
                              const uint8_t * gray0, const double * depth0, const uint8_t * gray1, const double * depth1,
                              double state[6], double rt[16], int * iterations_per_level )
{
  return guarded( [&]() {
    AnalyticType aligner;
    configure( aligner, cfg, k );
    aligner.SetSourceFrame( cv::Mat_< unsigned char >( h, w, gray0 ), cv::Mat_< double >( h, w, depth0 ) );
    aligner.SetTargetFrame( cv::Mat_< unsigned char >( h, w, gray1 ),
                            depth1 ? cv::Mat_< double >( h, w, depth1 ) : cv::Mat_< double >() );
    run( aligner, state, rt, iterations_per_level );
  } );
}

// Optimize of the Analytic class on level planes built by the caller (test hook): the pyramids are written into the
// object in place of SetSourceFrame / SetTargetFrame.
int phovo_ref_analytic_optimize_levels( const phovo_oracle_config * cfg, const double k[9], const phovo_oracle_level * levels,
                                        double state[6], double rt[16], int * iterations_per_level )
{
  return guarded( [&]() {
    AnalyticType aligner;
    configure( aligner, cfg, k );
    const int n = cfg->num_levels;
    aligner.m_IntensityPyramid0.resize( n );
    aligner.m_DepthPyramid0.resize( n );
    aligner.m_IntensityPyramid1.resize( n );
    aligner.m_IntensityGradientXPyramid1.resize( n );
    aligner.m_IntensityGradientYPyramid1.resize( n );
    for( int l = 0; l < n; l++ )
    {
      const phovo_oracle_level & lv = levels[l];
      aligner.m_IntensityPyramid0[l] = cv::Mat_< double >( lv.h, lv.w, lv.i0 );
      aligner.m_DepthPyramid0[l] = cv::Mat_< double >( lv.h, lv.w, lv.d0 );
      aligner.m_IntensityPyramid1[l] = cv::Mat_< double >( lv.h, lv.w, lv.i1 );
      aligner.m_IntensityGradientXPyramid1[l] = cv::Mat_< double >( lv.h, lv.w, lv.gx1 );
      aligner.m_IntensityGradientYPyramid1[l] = cv::Mat_< double >( lv.h, lv.w, lv.gy1 );
    }
    run( aligner, state, rt, iterations_per_level );
  } );
}

// The same for the BiObjective class; depth1 is required.
int phovo_ref_biobjective_align( const phovo_oracle_config * cfg, const double k[9], int w, int h,
                                 const uint8_t * gray0, const double * depth0, const uint8_t * gray1, const double * depth1,
                                 double state[6], double rt[16], int * iterations_per_level )
{
  return guarded( [&]() {
    BiObjectiveType aligner;
    configure( aligner, cfg, k );
    aligner.SetSourceFrame( cv::Mat_< unsigned char >( h, w, gray0 ), cv::Mat_< double >( h, w, depth0 ) );
    aligner.SetTargetFrame( cv::Mat_< unsigned char >( h, w, gray1 ), cv::Mat_< double >( h, w, depth1 ) );
    run( aligner, state, rt, iterations_per_level );
  } );
}

void phovo_ref_eigen_pose( const double state[6], double rt[16] )
{
  phovo::Numeric::Matrix44RowMajor< double > pose;
  phovo::eigenPose( state[0], state[1], state[2], state[3], state[4], state[5], pose );
  for( int i = 0; i < 4; i++ )
    for( int j = 0; j < 4; j++ )
      rt[ 4 * i + j ] = pose( i, j );
}

int phovo_ref_warp_image( const uint8_t * intensity, const double * depth, int w, int h, const double rt[16],
                          const double k[9], int level, uint8_t * warped )
{
  return guarded( [&]() {
    phovo::Numeric::Matrix44RowMajor< double > pose;
    phovo::Numeric::Matrix33RowMajor< double > intrinsics;
    for( int i = 0; i < 4; i++ )
      for( int j = 0; j < 4; j++ )
        pose( i, j ) = rt[ 4 * i + j ];
    for( int i = 0; i < 3; i++ )
      for( int j = 0; j < 3; j++ )
        intrinsics( i, j ) = k[ 3 * i + j ];
    cv::Mat_< unsigned char > out;
    phovo::warpImage( cv::Mat_< unsigned char >( h, w, intensity ), cv::Mat_< double >( h, w, depth ), out, pose, intrinsics,
                      level );
    std::memcpy( warped, out.ptr(), (std::size_t)w * (std::size_t)h );
  } );
}

} // extern "C"

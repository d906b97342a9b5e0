// Stand-in for <opencv2/imgproc/imgproc.hpp> (and the parts of core the reference reaches through it), written for this
// repository.  TEST INFRASTRUCTURE ONLY.  It is NOT OpenCV and holds none of its text.
//
// It provides the surface the reference's Gauss-Newton aligners use, so that their headers compile unmodified
// (oracle/Makefile.ref) where OpenCV is not installed:
//   cv::Mat_<T>     rows, cols, (r,c), (i), type(), zeros, convertTo; copies are shallow and share one buffer, as cv::Mat
//                   copies do (BuildPyramid's `imgAux = img` followed by an in-place blur depends on it)
//   cv::resize, cv::GaussianBlur, cv::Scharr, cv::mean, cv::absdiff
//   cv::FileStorage the values come from a registry that the driver fills; no file is read
//
// UNVERIFIED-vs-OpenCV: the arithmetic of resize, GaussianBlur, Scharr and convertTo is the oracle's restatement of
// OpenCV's behaviour (oracle/phovo_oracle.c, phovo_oracle_* plane functions), called from here, so that the reference
// build and the oracle see bit-identical pyramids.  cv::mean is a sequential sum divided by the count.  None of it has
// been compared with OpenCV.
#ifndef PHOVO_REF_STANDIN_OPENCV_IMGPROC
#define PHOVO_REF_STANDIN_OPENCV_IMGPROC

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <map>
#include <math.h>
#include <memory>
#include <string>
#include <vector>

#include "phovo_oracle.h"

namespace phovo_ref_standin
{
// What cv::FileStorage hands out: name of the yml key -> values.  Filled by the driver before ReadConfigurationFile.
extern thread_local std::map< std::string, std::vector< double > > settings;
[[noreturn]] void unsupported( const char * what );
}

namespace cv
{

typedef unsigned char uchar;

#ifndef CV_8U
#define CV_8U 0
#define CV_64F 6
#endif
enum { BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4 };
enum { INTER_LINEAR = 1 };

struct Size
{
  int width, height;
  Size() : width( 0 ), height( 0 ) {}
  Size( int w, int h ) : width( w ), height( h ) {}
};

struct Scalar
{
  double val[4];
  Scalar() { val[0] = val[1] = val[2] = val[3] = 0; }
};

template< class T > struct DepthOf;
template<> struct DepthOf< uchar > { enum { value = 0 }; };
template<> struct DepthOf< double > { enum { value = 6 }; };

template< class T >
class Mat_
{
  std::shared_ptr< std::vector< T > > m_buf;

public:
  int rows, cols;

  Mat_() : rows( 0 ), cols( 0 ) {}
  Mat_( int r, int c ) : m_buf( new std::vector< T >( (std::size_t)r * (std::size_t)c ) ), rows( r ), cols( c ) {}
  // deep copy of caller memory (the driver's way in)
  Mat_( int r, int c, const T * src ) : m_buf( new std::vector< T >( src, src + (std::size_t)r * (std::size_t)c ) ), rows( r ), cols( c ) {}

  void create( int r, int c )
  {
    if( m_buf && r == rows && c == cols ) return;        // same size: the buffer is kept, as cv::Mat::create keeps it
    m_buf.reset( new std::vector< T >( (std::size_t)r * (std::size_t)c ) );
    rows = r; cols = c;
  }

  static Mat_ zeros( int r, int c ) { return Mat_( r, c ); }  // std::vector value-initialises

  int type() const { return DepthOf< T >::value; }
  bool empty() const { return !m_buf || m_buf->empty(); }
  T * ptr() { return m_buf ? m_buf->data() : 0; }
  const T * ptr() const { return m_buf ? m_buf->data() : 0; }

  T & operator()( int r, int c ) { return ( *m_buf )[ (std::size_t)r * (std::size_t)cols + (std::size_t)c ]; }
  const T & operator()( int r, int c ) const { return ( *m_buf )[ (std::size_t)r * (std::size_t)cols + (std::size_t)c ]; }
  // one index on a 2-D continuous matrix: row i / cols, column i % cols, i.e. the linear element
  T & operator()( int i ) { return ( *m_buf )[ (std::size_t)i ]; }
  const T & operator()( int i ) const { return ( *m_buf )[ (std::size_t)i ]; }

  // u8 -> f64: phovo_oracle_convert_intensity (its factor is 1./255, the only one the reference passes);
  // f64 -> f64: element * alpha.
  template< class U >
  void convertTo( Mat_< U > & dst, int rtype, double alpha = 1, double beta = 0 ) const;
};

template<> template<>
inline void Mat_< uchar >::convertTo< double >( Mat_< double > & dst, int rtype, double alpha, double beta ) const
{
  if( rtype != 6 || alpha != 1. / 255 || beta != 0 ) phovo_ref_standin::unsupported( "convertTo(u8 -> f64) other than * 1./255" );
  dst.create( rows, cols );
  phovo_oracle_convert_intensity( ptr(), rows * cols, dst.ptr() );
}

template<> template<>
inline void Mat_< double >::convertTo< double >( Mat_< double > & dst, int rtype, double alpha, double beta ) const
{
  if( rtype != 6 || beta != 0 ) phovo_ref_standin::unsupported( "convertTo(f64 -> f64) with a type change or an offset" );
  Mat_< double > out( rows, cols );
  for( std::size_t i = 0; i < (std::size_t)rows * (std::size_t)cols; i++ ) out.ptr()[i] = ptr()[i] * alpha;
  dst = out;
}

// cv::resize(src, dst, Size(0,0), f, f) with f = 2^-L: phovo_oracle_resize_level, always into a fresh buffer
inline void resize( const Mat_< double > & src, Mat_< double > & dst, Size dsize, double fx = 0, double fy = 0,
                    int interpolation = INTER_LINEAR )
{
  int level = 0;
  double f = 1.0;
  while( f > fx && level < PHOVO_ORACLE_MAX_LEVELS ) { f = f / 2; level++; }
  if( dsize.width != 0 || dsize.height != 0 || fx != fy || f != fx || interpolation != INTER_LINEAR )
    phovo_ref_standin::unsupported( "resize other than Size(0,0) with equal power-of-two factors" );
  int lw, lh;
  phovo_oracle_level_size( src.cols, src.rows, level, &lw, &lh );
  Mat_< double > out( lh, lw );
  phovo_oracle_resize_level( src.ptr(), src.cols, src.rows, level, out.ptr() );
  dst = out;
}

// one pass of the oracle's Gaussian filter (sigma 3, reflect-101); in place when dst shares src's buffer
inline void GaussianBlur( const Mat_< double > & src, Mat_< double > & dst, Size ksize, double sigmaX, double sigmaY = 0,
                          int borderType = BORDER_DEFAULT )
{
  if( ksize.width != ksize.height || sigmaX != 3 || sigmaY != 0 || borderType != BORDER_DEFAULT )
    phovo_ref_standin::unsupported( "GaussianBlur other than a square kernel with sigma 3" );
  if( dst.ptr() == src.ptr() && dst.rows == src.rows && dst.cols == src.cols )
  {                                               // the reference's only use: blur in place, every alias sees it
    phovo_oracle_gaussian_blur_once( dst.ptr(), src.cols, src.rows, ksize.width );
    return;
  }
  Mat_< double > out( src.rows, src.cols, src.ptr() );
  phovo_oracle_gaussian_blur_once( out.ptr(), src.cols, src.rows, ksize.width );
  dst = out;
}

// cv::Scharr for (dx, dy) = (1, 0) or (0, 1): phovo_oracle_scharr computes both planes, the one asked for is kept
inline void Scharr( const Mat_< double > & src, Mat_< double > & dst, int ddepth, int dx, int dy, double scale = 1,
                    double delta = 0, int borderType = BORDER_DEFAULT )
{
  if( ddepth != 6 || delta != 0 || borderType != BORDER_DEFAULT || !( ( dx == 1 && dy == 0 ) || ( dx == 0 && dy == 1 ) ) )
    phovo_ref_standin::unsupported( "Scharr other than first derivatives in f64, delta 0, default border" );
  Mat_< double > gx( src.rows, src.cols ), gy( src.rows, src.cols );
  if( src.rows > 0 && src.cols > 0 )
    phovo_oracle_scharr( src.ptr(), src.cols, src.rows, scale, gx.ptr(), gy.ptr() );
  dst = dx ? gx : gy;
}

// sequential sum / count (UNVERIFIED-vs-OpenCV: its sum may unroll by four).  An empty matrix gives 0, as cv::mean does:
// the BiObjective gain of a level of zero pixels is then 0 / 0 = NaN.
inline Scalar mean( const Mat_< double > & src )
{
  Scalar out;
  double s = 0;
  const std::size_t n = (std::size_t)src.rows * (std::size_t)src.cols;
  for( std::size_t i = 0; i < n; i++ ) s += src.ptr()[i];
  out.val[0] = n ? s / (double)n : 0.0;
  return out;
}

inline void absdiff( const Mat_< double > & a, const Mat_< double > & b, Mat_< double > & dst )
{
  Mat_< double > out( a.rows, a.cols );
  for( std::size_t i = 0; i < (std::size_t)a.rows * (std::size_t)a.cols; i++ ) out.ptr()[i] = std::fabs( a.ptr()[i] - b.ptr()[i] );
  dst = out;
}

// ---- FileStorage: the driver's settings registry behind the reference's ReadConfigurationFile -------------------------
class FileNode
{
  const std::vector< double > * m_values;
public:
  explicit FileNode( const std::vector< double > * v ) : m_values( v ) {}
  const std::vector< double > & values( const char * what ) const
  {
    if( !m_values ) phovo_ref_standin::unsupported( what );
    return *m_values;
  }
};

inline void operator>>( const FileNode & n, int & v ) { v = (int)n.values( "missing integer setting" ).at( 0 ); }
inline void operator>>( const FileNode & n, bool & v ) { v = n.values( "missing boolean setting" ).at( 0 ) != 0; }
inline void operator>>( const FileNode & n, double & v ) { v = n.values( "missing real setting" ).at( 0 ); }
inline void operator>>( const FileNode & n, std::vector< double > & v ) { v = n.values( "missing real list" ); }
inline void operator>>( const FileNode & n, std::vector< int > & v )
{
  const std::vector< double > & s = n.values( "missing integer list" );
  v.resize( s.size() );
  for( std::size_t i = 0; i < s.size(); i++ ) v[i] = (int)s[i];
}

class FileStorage
{
public:
  enum { READ = 0 };
  FileStorage( const std::string &, int ) {}
  FileNode operator[]( const char * key ) const
  {
    std::map< std::string, std::vector< double > >::const_iterator it = phovo_ref_standin::settings.find( key );
    return FileNode( it == phovo_ref_standin::settings.end() ? 0 : &it->second );
  }
};

} // namespace cv

#endif

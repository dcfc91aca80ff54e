/* acn_variant.h -- kernel variant selection: runtime bools become compile-time constants, and a generic callable is called ONCE with
 * them, in the order given (instantiated true before false, the first argument outermost).  Plain C++17, no HIP.  A wrapper says
 *     acn_variant( f.count, f.prune, f.lds_nodes, [ & ]( auto C, auto P, auto L ) { hipLaunchKernelGGL( ( k< C.value, L.value, P.value > ), ... ); } );
 * and names its variant once, by its flags.  The variants of a kernel compute the same bits, so no GPU test can tell a transposed
 * pair: tests/test_variant_cpu.py checks that every constant arrives at the position it was passed in. */
#ifndef ACN_VARIANT_H
#define ACN_VARIANT_H
#include <type_traits>

template< class F > void acn_variant( bool a, F&& f ) { if( a ) f( std::true_type{} ); else f( std::false_type{} ); }
template< class F > void acn_variant( bool a, bool b, F&& f ) { acn_variant( a, [ & ]( auto A ) { acn_variant( b, [ & ]( auto B ) { f( A, B ); } ); } ); }
template< class F > void acn_variant( bool a, bool b, bool c, F&& f )
{
    acn_variant( a, [ & ]( auto A ) { acn_variant( b, c, [ & ]( auto B, auto C ) { f( A, B, C ); } ); } );
}

#endif

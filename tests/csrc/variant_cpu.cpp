/* actinon_amd/csrc/acn_variant.h on its own, twice.  As a shared library it is the extern "C" shim of tests/test_variant_cpu.py; with
 * -DVARIANT_CPU_MAIN it is a program that runs every combination itself, for the sanitizers.
 *
 * A call records what the callable received as  calls * 1000 + first * 100 + second * 10 + third  with the digit of a position 1
 * (false) or 2 (true), 0 for a position the form does not have: a transposed pair, a dropped or a doubled call all give another number. */
#include "acn_variant.h"

static int digit( bool v ) { return v ? 2 : 1; }

extern "C"
{
int vc_one( int a )
{
    int calls = 0, seen = 0;
    acn_variant( a != 0, [ & ]( auto A ) { constexpr bool av = A.value; calls++; seen = digit( av ) * 100; } );
    return calls * 1000 + seen;
}
int vc_pair( int a, int b )
{
    int calls = 0, seen = 0;
    acn_variant( a != 0, b != 0, [ & ]( auto A, auto B ) { constexpr bool av = A.value, bv = B.value; calls++; seen = digit( av ) * 100 + digit( bv ) * 10; } );
    return calls * 1000 + seen;
}
int vc_triple( int a, int b, int c )
{
    int calls = 0, seen = 0;
    acn_variant( a != 0, b != 0, c != 0, [ & ]( auto A, auto B, auto C ) {
        constexpr bool av = A.value, bv = B.value, cv = C.value;   /* constexpr: the values are usable as template arguments */
        calls++; seen = digit( av ) * 100 + digit( bv ) * 10 + digit( cv ); } );
    return calls * 1000 + seen;
}
}

#ifdef VARIANT_CPU_MAIN
#include <stdio.h>
int main()
{
    int bad = 0;
    for( int a = 0; a < 2; a++ )
    {
        bad += vc_one( a ) != 1000 + ( a + 1 ) * 100;
        for( int b = 0; b < 2; b++ )
        {
            bad += vc_pair( a, b ) != 1000 + ( a + 1 ) * 100 + ( b + 1 ) * 10;
            for( int c = 0; c < 2; c++ ) bad += vc_triple( a, b, c ) != 1000 + ( a + 1 ) * 100 + ( b + 1 ) * 10 + ( c + 1 );
        }
    }
    puts( bad ? "bad" : "ok" );
    return bad != 0;
}
#endif

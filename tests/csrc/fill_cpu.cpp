/* actinon_amd/csrc/acn_fill_host.h on its own: the extern "C" shim through which tests/test_fill_cpu.py calls the one check of
 * acn_fill_stats* -- the reading of a versioned acn_fill_params, the defaults, every refusal -- without a handle or a device. */
#include "acn_fill_host.h"

extern "C"
{
/* setup [ 5 ]: radius, normal_power_log2, no_demodulate, sigma_px, sigma_plane, written only when the call is accepted; msg only
 * when it is refused */
int fill_check( int have_handle, const void* stats, const void* surface, uint64_t width, uint64_t height, const void* prm, const void* out_stats,
                const void* out_need, uint32_t shard_world, double* setup, char* msg, size_t msg_room )
{
    std::string m;
    FillSetup su;
    const int st = acn_fill_check( have_handle != 0, stats, surface, ( size_t )width, ( size_t )height, ( const acn_fill_params* )prm, out_stats, out_need,
                                   shard_world, &su, &m );
    if( st == ACN_OK )
    {
        setup[ 0 ] = su.radius; setup[ 1 ] = su.normal_power_log2; setup[ 2 ] = su.no_demodulate; setup[ 3 ] = su.sigma_px; setup[ 4 ] = su.sigma_plane;
    }
    else if( msg && msg_room )
    {
        const size_t len = m.size() < msg_room - 1 ? m.size() : msg_room - 1;
        memcpy( msg, m.data(), len );
        msg[ len ] = 0;
    }
    return st;
}
}

/* acn_devbuf.h -- owners of what a handle and its runners hold on the device: a block of memory, an event, a stream.  Host-only and
 * without a HIP header: who allocates and releases is a policy (the HIP ones: acn_handle.h; tests/csrc/devbuf_cpu.cpp counts). */
#ifndef ACN_DEVBUF_H
#define ACN_DEVBUF_H

#include <cstddef>

/* A block of at least bytes() bytes, freed when the owner goes.  Mem: static int alloc( void** p, size_t want ), 0 when it worked, and
 * static void release( void* p ). */
template< class T, class Mem >
class Buf
{
    T* p_ = nullptr; size_t cap_ = 0;
public:
    Buf() = default;
    Buf( Buf&& o ) noexcept : p_( o.p_ ), cap_( o.cap_ ) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=( Buf&& o ) noexcept { if( this != &o ) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
    ~Buf() { reset(); }
    T* get() const { return p_; }   size_t bytes() const { return cap_; }
    void reset() { if( p_ ) Mem::release( p_ ); p_ = nullptr; cap_ = 0; }
    /* at least `want` bytes: grown, never shrunk, the contents not kept (the old block goes first); what Mem::alloc returned, and
     * after one that failed the block is null and holds 0 bytes */
    int grow( size_t want )
    {
        if( cap_ >= want ) return 0;
        reset();
        void* p = nullptr;
        const int st = Mem::alloc( &p, want );
        if( st == 0 ) { p_ = ( T* )p; cap_ = want; }
        return st;
    }
};

/* An object behind a handle value H (an event, a stream), destroyed once by Del::destroy( H ).  It is made in place:
 * create_call( x.put() ). */
template< class H, class Del >
class Owned
{
    H h_ = H();
public:
    Owned() = default;
    Owned( Owned&& o ) noexcept : h_( o.h_ ) { o.h_ = H(); }
    Owned& operator=( Owned&& o ) noexcept { if( this != &o ) { reset(); h_ = o.h_; o.h_ = H(); } return *this; }
    ~Owned() { reset(); }
    H get() const { return h_; }
    void reset() { if( h_ != H() ) Del::destroy( h_ ); h_ = H(); }
    H* put() { reset(); return &h_; }
};

#endif

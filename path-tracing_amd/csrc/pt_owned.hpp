// pt_owned.hpp -- one move-only owner for every resource of the handle that is not device memory (that is DevBuf, pt_runtime.hpp):
// events, streams, page-locked host memory.  Owned<H, Destroy> holds a handle value, calls Destroy on it exactly once -- when it
// goes out of scope, is released or is assigned over -- and can also hold a handle it must NOT destroy (borrow: the host's stream,
// the main stream standing in as the auxiliary one).  No HIP in here: pt_runtime.hpp names the aliases.
#pragma once

#include <utility>

template <typename H, auto Destroy> class Owned
{
    H h{};             // the value-initialised handle is "empty"
    bool mine = false; // Destroy is owed: set by adopt, never by borrow
public:
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(std::exchange(o.h, H{})), mine(std::exchange(o.mine, false)) {}
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o)
        {
            release();
            h = std::exchange(o.h, H{});
            mine = std::exchange(o.mine, false);
        }
        return *this;
    }
    ~Owned() { release(); }
    void adopt(H created) // takes ownership of a handle the caller has just created
    {
        release();
        h = created;
        mine = true;
    }
    void borrow(H others) // holds a handle that someone else destroys
    {
        release();
        h = others;
    }
    void release()
    {
        if (mine && h != H{})
            (void)Destroy(h);
        h = H{};
        mine = false;
    }
    H get() const { return h; }
    explicit operator bool() const { return h != H{}; }
};

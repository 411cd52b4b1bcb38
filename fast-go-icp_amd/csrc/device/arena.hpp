// The planner of a device arena (one_shot.hpp, the alignment scratch of ctx.hip): every array of a call or a feature in ONE allocation.
// No HIP in here: the layout is plain arithmetic (tests/test_arena_host.py builds this header alone).
#pragma once
#include <cstddef>
#include <vector>

namespace fgoicp {

// take() names an array once, in the order of the layout; every array starts on a 256-byte boundary.  place(), after the one
// allocation of total() bytes, sets the pointers; an array of no elements gets nullptr.
class Arena {
    struct Item {
        void* where;
        void (*set)(void* where, char* p);
        size_t at;
        bool empty;
    };
    std::vector<Item> items_;
    size_t total_ = 0;

  public:
    template <class T>
    void take(T*& p, size_t count) {
        items_.push_back({&p, [](void* where, char* at) { *static_cast<T**>(where) = reinterpret_cast<T*>(at); }, total_, count == 0});
        total_ += (sizeof(T) * count + 255) & ~(size_t)255;
    }
    size_t total() const { return total_; }
    void place(void* arena) const {
        for (const Item& it : items_) it.set(it.where, it.empty ? nullptr : static_cast<char*>(arena) + it.at);
    }
};

}  // namespace fgoicp

// philox_kat.cpp -- Philox4x32-10 of (counter, key) by an implementation that is not this project's: the round function
// of rocRAND's device header, called on the host.  No GPU, no HIP runtime call.  tests/test_stochastic_host.py compares
// the oracle's philox4x32(counter, key, 10) with what this prints, so that the generator the kernels, the host library
// and the oracle share is held to something none of them was written with.
//   hipcc --cuda-host-only -O1 tests/native/philox_kat.cpp -o build/philox_kat
//   build/philox_kat c0 c1 c2 c3 k0 k1 [c0 c1 c2 c3 k0 k1 ...]      (hex words; one line of four hex words per group)
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_philox4x32_10.h>

#include <cstdio>
#include <cstdlib>

struct Rounds : rocrand_device::philox4x32_10_engine {          // ten_rounds is a protected member
    uint4 operator()(uint4 counter, uint2 key) { return this->ten_rounds(counter, key); }
};

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 1) % 6 != 0) {
        std::fprintf(stderr, "usage: philox_kat c0 c1 c2 c3 k0 k1 [...]   (hex)\n");
        return 2;
    }
    Rounds rounds;
    for (int i = 1; i + 5 < argc; i += 6) {
        unsigned int w[6];
        for (int j = 0; j < 6; ++j) w[j] = (unsigned int)std::strtoul(argv[i + j], nullptr, 16);
        const uint4 r = rounds(uint4{w[0], w[1], w[2], w[3]}, uint2{w[4], w[5]});
        std::printf("%08x %08x %08x %08x\n", r.x, r.y, r.z, r.w);
    }
    return 0;
}

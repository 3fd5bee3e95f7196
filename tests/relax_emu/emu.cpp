// relax_kernel of abx_amd/csrc/relax.hip on CPU threads: emu_relax(args) checks the arguments through abx_relax itself, then runs the
// workgroups one after the other, 1024 threads each, on a 160 KB "LDS" that is filled with NaN bytes before every workgroup.  All pointers
// of the descriptor are host pointers.  relax_emu.hip = relax.hip with its dynamic-LDS declaration replaced by `emu_lds` (the test makes it).
#include <hip/hip_runtime.h>
thread_local EmuIdx threadIdx, blockIdx;
std::barrier<>* emu_block_barrier;
std::barrier<>* emu_wave_barrier[16];
double emu_shuffle[1024];
alignas(16) static unsigned char lds_store[160 * 1024];
unsigned char* emu_lds = lds_store;
#include "relax_emu.hip"
extern "C" int emu_relax(const AbxRelaxArgs* ap) {
    if (int rc = abx_relax(ap, nullptr, nullptr)) return rc;
    for (int b = 0; b < ap->B; ++b) {
        memset(lds_store, 0xff, sizeof(lds_store));
        std::barrier<> block(1024);
        emu_block_barrier = &block;
        std::vector<std::unique_ptr<std::barrier<>>> waves;
        for (int w = 0; w < 16; ++w) {
            waves.emplace_back(new std::barrier<>(64));
            emu_wave_barrier[w] = waves.back().get();
        }
        std::vector<std::thread> threads;
        for (int t = 0; t < 1024; ++t)
            threads.emplace_back([=] {
                threadIdx = EmuIdx{t, 0, 0};
                blockIdx = EmuIdx{b, 0, 0};
                relax_kernel(*ap);
            });
        for (auto& th : threads) th.join();
    }
    return 0;
}

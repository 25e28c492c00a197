// GPU test of the optimisers of the C++ API mirror: nn::SGD with momentum (dampening and weight decay; then Nesterov's form) and
// nn::Adam, two steps each on two small tensors with fixed gradients.  tests/test_gpu_optim.py compiles and runs this driver and
// compares the parameters it prints, by bit pattern, with tests/optim_ref.py and with the Python path (all end in
// gnnx_momentum_step_f32 / gnnx_adam_step_f32).
//   data:    p[k][i] = ((i * 37 + 11 * k) % 64 - 32) / 64;  gradient of step s: ((i * 29 + 7 * k + 13 * s) % 128 - 64) / 256
//   output:  one line per tensor, `<case><k> <n> <n hex words>`, cases sgd, nesterov, adam
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <valarray>
#include <vector>

#include "nn.h"
#include "tensor.h"

using namespace cyg;
using namespace std;

static const size_t kSizes[2] = {5, 1030};

static vector<tptr<float>> make_params()
{
    vector<tptr<float>> ps;
    for (size_t k = 0; k < 2; k++) {
        auto *v = new valarray<float>(kSizes[k]);
        for (size_t i = 0; i < kSizes[k]; i++) (*v)[i] = (float)((int)((i * 37 + 11 * k) % 64) - 32) / 64.0f;
        ps.push_back(make_shared<tensor<float>>(vector<size_t>{kSizes[k]}, v, true));
    }
    return ps;
}

static void set_grads(vector<tptr<float>> &ps, int s)
{
    for (size_t k = 0; k < 2; k++) {
        valarray<float> &g = *ps[k]->grad();
        for (size_t i = 0; i < kSizes[k]; i++) g[i] = (float)((int)((i * 29 + 7 * k + 13 * (size_t)s) % 128) - 64) / 256.0f;
    }
}

static void print_params(const char *name, vector<tptr<float>> &ps)
{
    for (size_t k = 0; k < 2; k++) {
        const valarray<float> &h = *ps[k]->cdata();
        printf("%s%zu %zu", name, k, h.size());
        for (size_t i = 0; i < h.size(); i++) {
            uint32_t w;
            memcpy(&w, &h[i], 4);
            printf(" %08X", w);
        }
        printf("\n");
    }
}

template <class Opt>
static void two_steps(const char *name, vector<tptr<float>> &ps, Opt &opt)
{
    for (int s = 0; s < 2; s++) {
        set_grads(ps, s);
        opt.step();
    }
    print_params(name, ps);
}

int main()
{
    try {
        {
            auto ps = make_params();
            nn::SGD opt(ps, 0.01f, 0.9f, 0.1f, 0.05f, false);
            two_steps("sgd", ps, opt);
        }
        {
            auto ps = make_params();
            nn::SGD opt(ps, 0.01f, 0.9f, 0.0f, 0.0f, true);
            two_steps("nesterov", ps, opt);
        }
        {
            auto ps = make_params();
            nn::Adam opt(ps, 0.01f, 0.9f, 0.999f);
            two_steps("adam", ps, opt);
        }
    } catch (const std::exception &e) {
        printf("FAIL %s\n", e.what());
        return 1;
    }
    return 0;
}

// GPU test of the masked loss and accuracy of the C++ API mirror: nn::cross_entropy_loss(logits, target, mask), its backward and
// nn::count_correct / nn::accuracy on a case file written by tests/test_gpu_masked.py, which compares the results with the Python
// path (both end in gnnx_softmax_ce_rows_f32 / gnnx_accuracy_rows_f32).
//   usage: test_host_masked_gpu <case file> <output directory>
//   case file: int32 n, c;  float32 logits[n * c];  int32 target[n];  uint8 mask[n]
//   outputs:   loss.bin (float32), grad.bin (float32 [n * c]), correct.bin (int64 correct, int64 masked rows)
#include <cstdint>
#include <cstdio>
#include <string>
#include <valarray>
#include <vector>

#include "graph.h"
#include "nn.h"
#include "tensor.h"

using namespace cyg;
using namespace std;

static bool write_file(const string &path, const void *p, size_t bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        printf("usage: %s <case file> <output directory>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[2];
    if (fread(hdr, sizeof(int32_t), 2, f) != 2) return 2;
    const size_t n = (size_t)hdr[0], c = (size_t)hdr[1];
    auto *lv = new valarray<float>(n * c);
    auto *tv = new valarray<int>(n);
    vector<uint8_t> mv(n);
    const bool ok = fread(&(*lv)[0], 4, n * c, f) == n * c && fread(&(*tv)[0], 4, n, f) == n && fread(mv.data(), 1, n, f) == n;
    fclose(f);
    if (!ok) return 2;
    try {
        auto logits = make_shared<tensor<float>>(vector<size_t>{n, c}, lv, true);
        auto target = make_shared<tensor<int>>(vector<size_t>{n}, tv, false);
        tensor<bool> mask(vector<size_t>{n}, false);
        int64_t masked = 0;
        for (size_t i = 0; i < n; i++) {
            (*mask.data())[i] = mv[i] != 0;
            masked += mv[i] != 0;
        }
        auto x = make_shared<tensor<float>>(vector<size_t>{n, 1}, 0.0f, false);
        graph::Data data(x);
        data.set_mask(mask, graph::DataType::TRAIN);

        auto loss = nn::cross_entropy_loss(logits, target, *data.train_mask());
        loss->backward();
        const float lossv = loss->item();
        const valarray<float> &g = *logits->grad();
        const int64_t counts[2] = {(int64_t)nn::count_correct(logits, target, *data.train_mask()), masked};
        const float acc = nn::accuracy(logits, target, *data.train_mask());
        if (acc != (float)counts[0] / (float)masked) {
            printf("FAIL accuracy %g != %lld / %lld\n", acc, (long long)counts[0], (long long)masked);
            return 1;
        }
        bool threw = false;   // a mask that selects nothing is an error, never a NaN loss
        tensor<bool> none(vector<size_t>{n}, false);
        try {
            nn::cross_entropy_loss(logits, target, none);
        } catch (const runtime_error &) {
            threw = true;
        }
        if (!threw) {
            printf("FAIL an empty mask did not throw\n");
            return 1;
        }
        const string dir = argv[2];
        if (!write_file(dir + "/loss.bin", &lossv, 4) || !write_file(dir + "/grad.bin", &g[0], 4 * n * c) ||
            !write_file(dir + "/correct.bin", counts, 16))
            return 2;
    } catch (const exception &e) {
        printf("FAIL threw: %s\n", e.what());
        return 1;
    }
    printf("masked host api (gpu) ok\n");
    return 0;
}

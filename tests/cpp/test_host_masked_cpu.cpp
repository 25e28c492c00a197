// CPU-side conventions of the label masks of graph::Data (no device call is made): set_mask stores a mask of one entry per vertex
// under its DataType and refuses any other size with the reference's message (reference src/graph.cpp:130-151, include/graph.h:14-19
// and :86-94), written against the same API.
#include <cstdio>
#include <cstring>
#include <functional>

#include "graph.h"
#include "nn.h"
#include "tensor.h"

using namespace cyg;
using namespace std;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);          \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static bool throws_with(const function<void()> &f, const char *msg)
{
    try {
        f();
    } catch (const runtime_error &e) {
        return strcmp(e.what(), msg) == 0;
    }
    return false;
}

int main()
{
    const size_t n = 5;
    auto x = make_shared<tensor<float>>(vector<size_t>{n, 3}, 1.0f, false);
    graph::Data data(x);
    CHECK(data.train_mask() == nullptr && data.val_mask() == nullptr && data.test_mask() == nullptr);

    tensor<bool> train(vector<size_t>{n}, false), val(vector<size_t>{n}, true), test(vector<size_t>{n}, false);
    (*train.data())[1] = true;
    data.set_mask(train);   // DataType::TRAIN is the default
    CHECK(data.train_mask() == &train && data.val_mask() == nullptr && data.test_mask() == nullptr);
    data.set_mask(val, graph::DataType::VAL);
    data.set_mask(test, graph::DataType::TEST);
    CHECK(data.train_mask() == &train && data.val_mask() == &val && data.test_mask() == &test);
    CHECK((*data.train_mask()->data())[1] && !(*data.train_mask()->data())[0]);
    CHECK(graph::DataType::TRAIN == 0 && graph::DataType::VAL == 1 && graph::DataType::TEST == 2);

    const char *msg = "invalid input, mask must be 1D and of same size with num of nodes in graph";
    tensor<bool> small(vector<size_t>{n - 1}, true), big(vector<size_t>{n, 2}, true);
    CHECK(throws_with([&] { data.set_mask(small); }, msg));
    CHECK(throws_with([&] { data.set_mask(big, graph::DataType::TEST); }, msg));
    CHECK(data.train_mask() == &train && data.test_mask() == &test);   // a refused mask replaces nothing

    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("masked host api (cpu) ok\n");
    return 0;
}

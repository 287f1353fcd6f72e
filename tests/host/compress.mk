# The host driver of the compressed encodings (tests/test_compress_host.py): a plain build and one under the sanitizer flags of the
# Makefile beside it ($(SAN)), which this file includes rather than repeats.   make -f compress.mk compress_host compress_host_san
include Makefile
ZDEPS = compress_host.cpp $(wildcard $(CSRC)/*.hpp)
compress_host: $(ZDEPS)
	$(CXX) -O2 -std=c++17 -w compress_host.cpp -o $@
compress_host_san: $(ZDEPS)
	$(CXX) $(SAN) compress_host.cpp -o $@

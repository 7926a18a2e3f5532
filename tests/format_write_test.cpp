// Test driver (no GPU): crafted records through the cleaners' writer (host/clean_common.h: RecordBatch::write) into a gzip file.
// usage: format_write_test <records> <out.gz>; <records> holds three entries per record -- header, read, quality -- each as
// "<len>\t<bytes>\n", so that an entry may hold any byte.
#include "clean_common.h"

static bool entry(FILE *f, string &s)
{
	size_t n = 0;
	if (fscanf(f, "%zu", &n) != 1 || fgetc(f) != '\t') return false;
	s.resize(n);
	if (n && fread(&s[0], 1, n, f) != n) return false;
	return fgetc(f) == '\n';
}

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 3;
	RecordBatch batch;
	string head, read, qual;
	while (entry(f, head)) {
		if (!entry(f, read) || !entry(f, qual)) return 4;
		batch.heads.push_back(head);
		batch.reads.push_back(read);
		batch.quals.push_back(qual);
	}
	fclose(f);
	GzWriter out(argv[2]);
	batch.write(out);
	out.close();
	printf("%zu\n", batch.size());
	return 0;
}
